// Signal-level scores next to the path (loss/sdr.py:104-215, 263-330 of mcw519/PureSound): every SDR / SI-SNR variant
// of the reference is a function of five moments of the (estimate, reference) pair -- sum a, sum b, sum a^2, sum b^2,
// sum ab over the time axis -- so one streaming pass over the two waveforms replaces the reference's chain of
// mean / subtract / multiply / sum passes (zero-mean, projection and error signal are algebra on the moments, done in
// fp64 by the caller).  HBM-bound: 8 bytes per sample pair; fp64 accumulation, partials per workgroup (no atomics,
// deterministic), reduced by the caller.
#include "ps_common.h"

namespace ps {

constexpr int WM_CHUNK = 8192;  // samples per workgroup

// ROWS: row n ends at len_rows[n] <= L samples and may hold anything behind them (ps_wave_moments_rows_f64).  A chunk at or
// behind the row's end loads nothing and writes its slot as zeros; the chunks in front of it sum in the order of the
// whole-row kernel, so that len_rows[n] == L gives its bits.
template <bool ROWS>
__global__ __launch_bounds__(256) void wave_moments_kernel(const float* a, const float* b, const int* len_rows, double* out,
                                                           int L, int lda, int ldb, int chunks) {
  __shared__ double red[8 * 5];
  const int n = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const float* pa = a + (size_t)n * lda;
  const float* pb = b + (size_t)n * ldb;
  const int len = ROWS ? row_limit(len_rows, n, L) : L;
  const int lo = c * WM_CHUNK, hi = lo + WM_CHUNK < len ? lo + WM_CHUNK : len;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  // fp32 products are exact in fp64; four independent chains per thread keep the loads in flight
  for (int i = lo + tid; i < hi; i += 256) {
    const double x = pa[i], y = pb[i];
    s[0] += x;
    s[1] += y;
    s[2] += x * x;
    s[3] += y * y;
    s[4] += x * y;
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double v = wave_sum(s[k]);
    if (lane == 0) red[wave * 5 + k] = v;
  }
  __syncthreads();
  if (tid < 5) out[((size_t)n * chunks + c) * 5 + tid] = red[tid] + red[5 + tid] + red[10 + tid] + red[15 + tid];
}

}  // namespace ps

extern "C" int ps_wave_moments_chunks(int L) { return L <= 0 ? 0 : (L + ps::WM_CHUNK - 1) / ps::WM_CHUNK; }

static int wave_moments_check(const char* who, const float* a, const float* b, const double* partials, int N, int L, int lda,
                              int ldb) {
  if (!a || !b || !partials || N <= 0 || L <= 0 || lda < L || ldb < L || N > 65535) {
    ps::set_error("%s: null pointer or bad size (N=%d L=%d lda=%d ldb=%d)", who, N, L, lda, ldb);
    return PS_E_INVALID;
  }
  return 0;
}

extern "C" int ps_wave_moments_f64(const float* a, const float* b, double* partials, int N, int L, int lda, int ldb,
                                   void* stream) {
  using namespace ps;
  if (const int rc = wave_moments_check("ps_wave_moments_f64", a, b, partials, N, L, lda, ldb)) return rc;
  const int chunks = ps_wave_moments_chunks(L);
  {
    LaunchTimer timer("wave_moments", (hipStream_t)stream);
    hipLaunchKernelGGL(wave_moments_kernel<false>, dim3(chunks, N), dim3(256), 0, (hipStream_t)stream, a, b, nullptr, partials,
                       L, lda, ldb, chunks);
  }
  return launch_status("ps_wave_moments_f64");
}

extern "C" int ps_wave_moments_rows_f64(const float* a, const float* b, const int* len_rows, double* partials, int N, int L,
                                        int lda, int ldb, void* stream) {
  using namespace ps;
  if (const int rc = wave_moments_check("ps_wave_moments_rows_f64", a, b, partials, N, L, lda, ldb)) return rc;
  if (!len_rows) {
    set_error("ps_wave_moments_rows_f64: len_rows is NULL");
    return PS_E_INVALID;
  }
  const int chunks = ps_wave_moments_chunks(L);
  {
    LaunchTimer timer("wave_moments_rows", (hipStream_t)stream);
    hipLaunchKernelGGL(wave_moments_kernel<true>, dim3(chunks, N), dim3(256), 0, (hipStream_t)stream, a, b, len_rows, partials,
                       L, lda, ldb, chunks);
  }
  return launch_status("ps_wave_moments_rows_f64");
}
