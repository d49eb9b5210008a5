// Spectral scores next to the path (loss/stft_loss.py of mcw519/PureSound: STFTLoss, MultiResolutionSTFTLoss,
// over_suppression_loss).  Every score is algebra on four sums over the frames and bins of the clamped magnitude
// spectrograms x (estimate) and y (reference) -- sum (y-x)^2, sum y^2, sum |log y - log x|, sum relu(y^p - x^p)^2 -- done in
// fp64 by the caller.  torch.stft(center=True, reflect) with a fixed window is a dense product against a windowed Fourier
// basis, so it runs on ps_conv1x1_f32 (exact fp32 products) over the window's support only; this file holds the two
// byte-moving steps around that product: the reflecting framing in front of it and the pair reduction behind it.
#include "ps_common.h"

namespace ps {

// frames[r][k][t] = wav[r][reflect(t*hop + k + off - n_fft/2)], k < win, off = (n_fft - win)/2: the window's support of
// torch.stft's frame t (the signal reflect-padded by n_fft/2 on both sides, the window centred in n_fft samples).  One
// reflection is enough: L > n_fft/2 and T = 1 + (L + 2 (n_fft/2) - n_fft) / hop frames (one fewer for an odd n_fft when hop
// divides L) keep every index in [-(n_fft/2), L + n_fft/2 - 1]; the entry refuses any other T.  Rows r < N come from a, rows N + r from b.  One thread per (k, 4 frames): 16-byte
// coalesced stores, gathered dword loads; zeros in the pad columns t >= T.
// ROWS (ps_frame_reflect_rows_f32): rows n and N + n hold len_rows[n] <= L samples and anything behind them; the row is framed
// as an utterance of that length on its own -- T_n = 1 + (L_n - n_fft % 2) / hop frames, reflected at the row's OWN end -- and
// columns T_n <= t < ldt are zeros.  The bound above holds with (L_n, T_n) in the place of (L, T); a limit at or below n_fft/2,
// which the host refuses, frames nothing (T_n = 0), so that no index leaves the row whatever the array holds.
template <bool ROWS>
__global__ __launch_bounds__(256) void frame_reflect_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const int* __restrict__ len_rows, float* __restrict__ frames,
                                                            int N, int L, int lda, int ldb, int shift, int win, int hop,
                                                            int n_fft, int T, int ldt) {
  const int r = blockIdx.z, k = blockIdx.y;
  const int t = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (t >= ldt) return;
  const float* x = r < N ? a + (size_t)r * lda : b + (size_t)(r - N) * ldb;
  if constexpr (ROWS) {
    L = row_limit(len_rows, r < N ? r : r - N, L);
    T = L > n_fft / 2 ? 1 + (L - n_fft % 2) / hop : 0;   // <= the launch-wide T
  }
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    long long p = (long long)(t + e) * hop + k + shift;   // shift = off - n_fft/2
    if (p < 0) p = -p;
    if (p >= L) p = 2LL * (L - 1) - p;
    if (t + e >= T) p = 0;   // a pad column: no sample behind it
    v[e] = (t + e < T) ? x[p] : 0.f;
  }
  *reinterpret_cast<f32x4*>(frames + ((size_t)r * win + k) * ldt + t) = v;
}

// sqrt(clamp(re^2 + im^2, min=1e-7)) (stft_loss.py:24; a NaN stays a NaN).  One spelled-out fused multiply-add for estimate and
// reference alike: left to the compiler's contraction the two could round differently, and identical signals must score 0.
__device__ __forceinline__ float clamped_magnitude(float re, float im) {
  const float p = __builtin_fmaf(re, re, im * im);
  return sqrtf(p < 1e-7f ? 1e-7f : p);
}

constexpr int SPM_BINS = 16;     // bins per workgroup: 4 per wave
constexpr int SPM_FRAMES = 256;  // frames per workgroup: 4 per lane

// One workgroup: SPM_BINS bins x SPM_FRAMES frames of utterance n; each lane reads 4 frames of (re, im) of the estimate
// (row n) and of the reference (row N + n) as 16-byte loads.  Magnitudes in fp32 as the reference forms them, everything
// behind them in fp64; frames t >= T and bins >= bins are selected out, never multiplied out (a NaN there changes no bit).
// The four sums of the workgroup go to its own slot of partials [N][parts][4], in a fixed order.
// ROWS (ps_spec_pair_moments_rows_f64): utterance n holds t_rows[n] <= T frames; lanes whose four frames lie at or behind them
// load nothing, so a workgroup entirely behind them writes its slot as zeros without a load, and the frames in front of them
// sum in the order of the whole-row kernel (t_rows[n] == T gives its bits).  No `mag`.
template <bool ROWS>
__global__ __launch_bounds__(256) void spec_pair_moments_kernel(const float* __restrict__ spec, const int* __restrict__ t_rows,
                                                                double* __restrict__ partials, float* __restrict__ mag, int N,
                                                                int bins, int T, int ldt, int tchunks, double p) {
  __shared__ double red[4 * 4];
  const int n = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int b0 = (part / tchunks) * SPM_BINS, t = (part % tchunks) * SPM_FRAMES + lane * 4;
  const size_t rows = 2 * (size_t)bins;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (ROWS) T = row_limit(t_rows, n, T);
  if (ROWS ? t < T : t < ldt) {
#pragma unroll
    for (int j = 0; j < SPM_BINS / 4; ++j) {
      const int bin = b0 + wave + 4 * j;
      if (bin >= bins) break;
      const size_t xe = ((size_t)n * rows + bin) * ldt + t, ye = (((size_t)N + n) * rows + bin) * ldt + t;
      const f32x4 xr = *reinterpret_cast<const f32x4*>(spec + xe);
      const f32x4 xi = *reinterpret_cast<const f32x4*>(spec + xe + (size_t)bins * ldt);
      const f32x4 yr = *reinterpret_cast<const f32x4*>(spec + ye);
      const f32x4 yi = *reinterpret_cast<const f32x4*>(spec + ye + (size_t)bins * ldt);
      f32x4 mx, my;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool live = t + e < T;
        mx[e] = live ? clamped_magnitude(xr[e], xi[e]) : 0.f;
        my[e] = live ? clamped_magnitude(yr[e], yi[e]) : 0.f;
        if (live) {
          const double x = mx[e], y = my[e];
          const double lx = log(x), ly = log(y), d = y - x;
          const double yp = p == 0.5 ? sqrt(y) : (p == 1.0 ? y : exp(p * ly));
          const double xp = p == 0.5 ? sqrt(x) : (p == 1.0 ? x : exp(p * lx));
          const double o = yp > xp ? yp - xp : 0.0;
          s[0] += d * d;
          s[1] += y * y;
          s[2] += fabs(ly - lx);
          s[3] += o * o;
        }
      }
      if (!ROWS && mag) {
        *reinterpret_cast<f32x4*>(mag + ((size_t)n * bins + bin) * ldt + t) = mx;
        *reinterpret_cast<f32x4*>(mag + (((size_t)N + n) * bins + bin) * ldt + t) = my;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum(s[k]);
    if (lane == 0) red[wave * 4 + k] = v;
  }
  __syncthreads();
  if (tid < 4) partials[((size_t)n * gridDim.x + part) * 4 + tid] = red[tid] + red[4 + tid] + red[8 + tid] + red[12 + tid];
}

}  // namespace ps

using namespace ps;

// The two framing entries: one check, one launch (len_rows == NULL: whole rows)
static int frame_reflect(const char* who, const float* a, const float* b, const int* len_rows, float* frames, int N, int L,
                         int lda, int ldb, int n_fft, int win, int hop, int T, int ldt, void* stream) {
  const int rows = b ? 2 * N : N;
  if (!a || !frames || N <= 0 || N > 32767 || n_fft <= 0 || win <= 0 || win > n_fft || win > 65535 || hop <= 0 ||
      L <= n_fft / 2 || lda < L || (b && ldb < L) || T != 1 + (L - n_fft % 2) / hop || ldt < T || ldt % kTileT != 0 ||
      ((uintptr_t)frames & 15)) {
    set_error("%s: bad argument (N=%d L=%d lda=%d ldb=%d n_fft=%d win=%d hop=%d T=%d ldt=%d; reflect "
              "padding needs L > n_fft/2)", who, N, L, lda, ldb, n_fft, win, hop, T, ldt);
    return PS_E_INVALID;
  }
  const dim3 grid((ldt / 4 + 255) / 256, win, rows);
  const int shift = (n_fft - win) / 2 - n_fft / 2;
  {
    LaunchTimer timer(len_rows ? "frame_reflect_rows" : "frame_reflect", (hipStream_t)stream);
    if (len_rows)
      hipLaunchKernelGGL(frame_reflect_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a, b, len_rows, frames, N, L, lda,
                         ldb, shift, win, hop, n_fft, T, ldt);
    else
      hipLaunchKernelGGL(frame_reflect_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a, b, nullptr, frames, N, L, lda,
                         ldb, shift, win, hop, n_fft, T, ldt);
  }
  return launch_status(who);
}

extern "C" int ps_frame_reflect_f32(const float* a, const float* b, float* frames, int N, int L, int lda, int ldb, int n_fft,
                                    int win, int hop, int T, int ldt, void* stream) {
  return frame_reflect("ps_frame_reflect_f32", a, b, nullptr, frames, N, L, lda, ldb, n_fft, win, hop, T, ldt, stream);
}

extern "C" int ps_frame_reflect_rows_f32(const float* a, const float* b, const int* len_rows, float* frames, int N, int L,
                                         int lda, int ldb, int n_fft, int win, int hop, int T, int ldt, void* stream) {
  if (!len_rows) {
    set_error("ps_frame_reflect_rows_f32: len_rows is NULL");
    return PS_E_INVALID;
  }
  return frame_reflect("ps_frame_reflect_rows_f32", a, b, len_rows, frames, N, L, lda, ldb, n_fft, win, hop, T, ldt, stream);
}

extern "C" int ps_spec_pair_moments_parts(int bins, int T) {
  if (bins <= 0 || T <= 0) return 0;
  const long long parts = (long long)((bins + SPM_BINS - 1) / SPM_BINS) * ((T + SPM_FRAMES - 1) / SPM_FRAMES);
  return parts > 0x7fffffffLL ? 0 : (int)parts;
}

// The two reduction entries: one check, one launch (t_rows == NULL: whole rows)
static int spec_pair_moments(const char* who, const float* spec, const int* t_rows, double* partials, float* mag, int N, int bins,
                             int T, int ldt, double p, void* stream) {
  const int parts = ps_spec_pair_moments_parts(bins, T);
  if (!spec || !partials || N <= 0 || N > 32767 || parts <= 0 || ldt < T || ldt % kTileT != 0 || !(p > 0.0) || !(p < 64.0) ||
      ((uintptr_t)spec & 15) || ((uintptr_t)mag & 15)) {
    set_error("%s: bad argument (N=%d bins=%d T=%d ldt=%d p=%g)", who, N, bins, T, ldt, p);
    return PS_E_INVALID;
  }
  const int tchunks = (T + SPM_FRAMES - 1) / SPM_FRAMES;
  {
    LaunchTimer timer(t_rows ? "spec_pair_moments_rows" : "spec_pair_moments", (hipStream_t)stream);
    if (t_rows)
      hipLaunchKernelGGL(spec_pair_moments_kernel<true>, dim3(parts, N), dim3(256), 0, (hipStream_t)stream, spec, t_rows, partials,
                         nullptr, N, bins, T, ldt, tchunks, p);
    else
      hipLaunchKernelGGL(spec_pair_moments_kernel<false>, dim3(parts, N), dim3(256), 0, (hipStream_t)stream, spec, nullptr,
                         partials, mag, N, bins, T, ldt, tchunks, p);
  }
  return launch_status(who);
}

extern "C" int ps_spec_pair_moments_f64(const float* spec, double* partials, float* mag, int N, int bins, int T, int ldt,
                                        double p, void* stream) {
  return spec_pair_moments("ps_spec_pair_moments_f64", spec, nullptr, partials, mag, N, bins, T, ldt, p, stream);
}

extern "C" int ps_spec_pair_moments_rows_f64(const float* spec, const int* t_rows, double* partials, int N, int bins, int T,
                                             int ldt, double p, void* stream) {
  if (!t_rows) {
    set_error("ps_spec_pair_moments_rows_f64: t_rows is NULL");
    return PS_E_INVALID;
  }
  return spec_pair_moments("ps_spec_pair_moments_rows_f64", spec, t_rows, partials, nullptr, N, bins, T, ldt, p, stream);
}
