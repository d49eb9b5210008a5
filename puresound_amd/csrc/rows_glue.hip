// Row-wise glue between the GEMMs and the recurrences of the recurrent maskers (DPRNN, SkiM, DPCRN / DPARN) and the
// gated TCN, on the padded channel-major layout [N][C][ldt]: no entry here carries state from one frame to the next.
//   ps_chan_layernorm_f32    nn.LayerNorm(C) / ChanLN over the channels of each frame with the residual add, PReLU,
//                            sigmoid and gating product that follow it in the reference; dprnn.py:157-172,
//                            skim.py:85-98,226, lobe/trivial.py:61-126,160
//   ps_film_apply_f32        FiLM modulation scale * x + bias; lobe/trivial.py:162-167
//   ps_lstm_cell_f32         one LSTM cell update per (unit, frame) from complete gate pre-activations (streaming step)
//   ps_unfold_taps(_out)_f32, ps_gated_product_f32, ps_segment_overlap_f32   the GatedTCN pieces, 50 % overlapped segmentation
#include "ps_common.h"

namespace ps {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---- LayerNorm over channels ---------------------------------------------------------------------------------
struct ClnArgs {
  const float* x;
  const float* gamma;
  const float* beta;
  const float* res;
  const float* slope;
  const float* mul;
  float* y;
  float eps;
  int sigmoid;
  int C, T, ldt;
};

// 64 frames x 4 channel quarters per workgroup; three passes over the (L1/L2 resident) 64 x C tile: mean,
// centred second moment (the reference's two-pass variance), normalise + epilogue.
template <int PARTS>
__global__ __launch_bounds__(64 * PARTS) void chan_layernorm_kernel(ClnArgs a) {
  __shared__ float red[PARTS][64];
  const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane, n = blockIdx.y;
  const bool live = t < a.T;
  const size_t base = (size_t)n * a.C * a.ldt + (live ? t : 0);
  float s = 0.f;
  for (int ch = part; ch < a.C; ch += PARTS) s += live ? a.x[base + (size_t)ch * a.ldt] : 0.f;
  red[part][lane] = s;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int p = 0; p < PARTS; ++p) tot += red[p][lane];
  const float mean = tot / (float)a.C;
  __syncthreads();
  float q = 0.f;
  for (int ch = part; ch < a.C; ch += PARTS) {
    const float dv = live ? a.x[base + (size_t)ch * a.ldt] - mean : 0.f;
    q += dv * dv;
  }
  red[part][lane] = q;
  __syncthreads();
  tot = 0.f;
#pragma unroll
  for (int p = 0; p < PARTS; ++p) tot += red[p][lane];
  const float var = tot / (float)a.C;
  const float rstd = 1.f / sqrtf(var + a.eps);
  if (!live) return;
  const float slope = a.slope ? a.slope[0] : 1.f;
  for (int ch = part; ch < a.C; ch += PARTS) {
    const size_t off = base + (size_t)ch * a.ldt;
    float v = (a.x[off] - mean) * rstd * a.gamma[ch] + a.beta[ch];
    if (a.slope) v = prelu(v, slope);
    if (a.sigmoid) v = sigmoidf_(v);
    if (a.mul) v *= a.mul[off];
    if (a.res) v += a.res[off];
    a.y[off] = v;
  }
}

// The same for C <= 4 * CPT with the thread's channels held in registers: one pass over x instead of three (on the 2-D maps
// of DPCRN / DPARN -- 32 x 32,745 frames x 128 channels -- the three passes ran at 2 TB/s of useful traffic, 770 us).  Sums in the
// order of chan_layernorm_kernel<4>: identical results.
template <int CPT>
__global__ __launch_bounds__(256) void chan_layernorm_reg_kernel(ClnArgs a) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane, n = blockIdx.y;
  const bool live = t < a.T;
  const size_t base = (size_t)n * a.C * a.ldt + (live ? t : 0);
  float v[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int ch = part + 4 * i;
    v[i] = (live && ch < a.C) ? a.x[base + (size_t)ch * a.ldt] : 0.f;
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) s += v[i];
  red[part][lane] = s;
  __syncthreads();
  const float mean = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (float)a.C;
  __syncthreads();
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const float dv = (live && part + 4 * i < a.C) ? v[i] - mean : 0.f;
    q += dv * dv;
  }
  red[part][lane] = q;
  __syncthreads();
  const float var = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (float)a.C;
  const float rstd = 1.f / sqrtf(var + a.eps);
  if (!live) return;
  const float slope = a.slope ? a.slope[0] : 1.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int ch = part + 4 * i;
    if (ch < a.C) {
      const size_t off = base + (size_t)ch * a.ldt;
      float o = (v[i] - mean) * rstd * a.gamma[ch] + a.beta[ch];
      if (a.slope) o = prelu(o, slope);
      if (a.sigmoid) o = sigmoidf_(o);
      if (a.mul) o *= a.mul[off];
      if (a.res) o += a.res[off];
      a.y[off] = o;
    }
  }
}

// One LSTM cell update per (unit, frame) from complete gate pre-activations (the streaming step: the recurrent
// product W_hh h is part of the gates GEMM there, its K axis being [x; h]).
__global__ __launch_bounds__(256) void lstm_cell_kernel(const float* __restrict__ gates, float* __restrict__ c,
                                                        float* __restrict__ h, int H, int T, int ldg, int lds_) {
  const int t = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int nd = blockIdx.z;  // utterance * directions + direction
  if (t >= T || j >= H) return;
  const float* g = gates + ((size_t)nd * 4 * H + j) * ldg + t;
  const size_t so = ((size_t)nd * H + j) * lds_ + t;
  const float gi = sigmoidf_(g[0]);
  const float gf = sigmoidf_(g[(size_t)H * ldg]);
  const float gg = tanhf(g[(size_t)2 * H * ldg]);
  const float go = sigmoidf_(g[(size_t)3 * H * ldg]);
  const float cn = gf * c[so] + gi * gg;
  c[so] = cn;
  h[so] = go * tanhf(cn);
}

__global__ __launch_bounds__(256) void film_apply_kernel(const float* __restrict__ x, const float* __restrict__ sb,
                                                         float* __restrict__ y, int C, int T, int ldt) {
  const int t = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int ch = blockIdx.y, n = blockIdx.z;
  if (t >= T) return;
  const size_t xo = ((size_t)n * C + ch) * ldt + t;
  const size_t so = ((size_t)n * 2 * C + ch) * ldt + t;
  const size_t bo = so + (size_t)C * ldt;
  const f32x4 xv = *reinterpret_cast<const f32x4*>(x + xo);
  const f32x4 sv = *reinterpret_cast<const f32x4*>(sb + so);
  const f32x4 bv = *reinterpret_cast<const f32x4*>(sb + bo);
  *reinterpret_cast<f32x4*>(y + xo) = sv * xv + bv;
}

// ---- GatedTCN pieces (conv_tasnet.py:129-215) -----------------------------------------------------------------
// Unfold a dense dilated convolution into a 1x1 one: row (j, k) of the output is input channel k shifted by tap j
// (zero outside [0, T)), so W[m][k][j] becomes a plain [M][P*Kc] matrix for ps_conv1x1_f32.  Optional per-(utterance,
// channel) FiLM scale/shift applied before the zero padding, and E constant embedding rows appended per tap (the
// reference concatenates the repeated embedding BEFORE F.conv1d pads, so its taps drop out at the edges too).
__global__ __launch_bounds__(256) void unfold_taps_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          const float* __restrict__ embed, int K, int E, int T, int T_out,
                                                          int ldt, int P, int dilation, int left) {
  // T = valid input frames, T_out >= T = output frames (the causal gated block of the reference pads both sides and
  // trims only after its output conv: its norms see T + padding frames, conv_tasnet.py:203-211)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int row = blockIdx.y;  // j * (K + E) + k
  const int n = blockIdx.z;
  const int Kc = K + E;
  const int j = row / Kc, k = row % Kc;
  if (t >= T_out) return;
  const int src = t + j * dilation - left;
  float v = 0.f;
  if (src >= 0 && src < T) {
    if (k < K) {
      v = x[((size_t)n * K + k) * ldt + src];
      if (scale) v = v * scale[(size_t)n * K + k] + shift[(size_t)n * K + k];
    } else {
      v = embed[(size_t)n * E + (k - K)];
    }
  }
  y[((size_t)n * P * Kc + row) * ldt + t] = v;
}

struct GateArgs {
  const float* l;
  const float* r;
  float* y;
  ps_prologue pl, pr;
  int H, T, ldt;
};

// y = PReLU(norm(l)) * sigmoid(PReLU(norm(r))): the two branch tails of the gated block, norms gLN / folded bN1d.
__global__ __launch_bounds__(256) void gated_product_kernel(GateArgs a) {
  __shared__ double red[8];
  const int n = blockIdx.z, ch = blockIdx.y;
  const NormScalars nl = load_norm_scalars(a.pl, n, red);
  const NormScalars nr = load_norm_scalars(a.pr, n, red);
  const int t = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (t >= a.T) return;
  const float scl = a.pl.norm != PS_NORM_NONE ? a.pl.gamma[ch] * nl.rstd : 1.f;
  const float shl = (a.pl.norm != PS_NORM_NONE ? a.pl.beta[ch] : 0.f) - nl.mean * scl;
  const float scr = a.pr.norm != PS_NORM_NONE ? a.pr.gamma[ch] * nr.rstd : 1.f;
  const float shr = (a.pr.norm != PS_NORM_NONE ? a.pr.beta[ch] : 0.f) - nr.mean * scr;
  const float sl = a.pl.prelu ? a.pl.slope[0] : 1.f, sr = a.pr.prelu ? a.pr.slope[0] : 1.f;
  const size_t off = ((size_t)n * a.H + ch) * a.ldt + t;
  const f32x4 lv = *reinterpret_cast<const f32x4*>(a.l + off);
  const f32x4 rv = *reinterpret_cast<const f32x4*>(a.r + off);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lf = prelu(lv[e] * scl + shl, sl);
    const float rf = prelu(rv[e] * scr + shr, sr);
    o[e] = lf * sigmoidf_(rf);
  }
  *reinterpret_cast<f32x4*>(a.y + off) = o;
}

// ---- 50 % overlapped segmentation (SplitMerge.split / merge, lobe/trivial.py:178-241; SkiM.split / merge) ------------
// mode 0 (split): dst frame s*K + k <- src frame (s/2)*K + k + (s&1)*K/2 - K/2 (zero outside [0, T_src))
// mode 1 (merge): dst frame t <- (src[even cover] + src[odd cover]) / 2
__global__ __launch_bounds__(256) void segment_overlap_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                              int T_src, int ld_src, int T_dst, int ld_dst, int K,
                                                              int mode) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  const size_t row = blockIdx.y;
  if (f >= T_dst) return;
  const float* s = src + row * ld_src;
  const int stride = K / 2;
  float v;
  if (mode == 0) {
    const int seg = f / K, k = f % K;
    const int t = (seg >> 1) * K + k + (seg & 1) * stride - stride;
    v = (t >= 0 && t < T_src) ? s[t] : 0.f;
  } else {
    const int e = stride + f;
    const int fa = (2 * (e / K)) * K + e % K;
    const int fb = (2 * (f / K) + 1) * K + f % K;
    v = (s[fa] + s[fb]) * 0.5f;
  }
  dst[row * ld_dst + f] = v;
}

}  // namespace ps

using namespace ps;

extern "C" int ps_chan_layernorm_f32(const float* x, const float* gamma, const float* beta, float eps,
                                     const float* prelu_slope, int sigmoid, const float* mul, const float* res,
                                     float* y, int N, int C, int T, int ldt, void* stream) {
  if (!x || !gamma || !beta || !y || N <= 0 || C <= 0 || T <= 0 || ldt < T || N > 65535) {
    set_error("ps_chan_layernorm_f32: bad argument (N=%d C=%d T=%d ldt=%d)", N, C, T, ldt);
    return PS_E_INVALID;
  }
  ClnArgs a{x, gamma, beta, res, prelu_slope, mul, y, eps, sigmoid, C, T, ldt};
  {
    LaunchTimer timer("chan_layernorm", (hipStream_t)stream);
    // few frames (streaming step, state rows): split the channels 16 ways instead of 4 to shorten the serial walk
    if ((long long)((T + 63) / 64) * N < 64)
      hipLaunchKernelGGL((chan_layernorm_kernel<16>), dim3((T + 63) / 64, N), dim3(1024), 0, (hipStream_t)stream, a);
    else if (C <= 64 && !dbg(PS_DBG_CHAN_LN_THREE_PASS))  // (else the three-pass kernel; tests run both)
      hipLaunchKernelGGL((chan_layernorm_reg_kernel<16>), dim3((T + 63) / 64, N), dim3(256), 0, (hipStream_t)stream, a);
    else if (C <= 128 && !dbg(PS_DBG_CHAN_LN_THREE_PASS))
      hipLaunchKernelGGL((chan_layernorm_reg_kernel<32>), dim3((T + 63) / 64, N), dim3(256), 0, (hipStream_t)stream, a);
    else if (C <= 256 && !dbg(PS_DBG_CHAN_LN_THREE_PASS))
      hipLaunchKernelGGL((chan_layernorm_reg_kernel<64>), dim3((T + 63) / 64, N), dim3(256), 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL((chan_layernorm_kernel<4>), dim3((T + 63) / 64, N), dim3(256), 0, (hipStream_t)stream, a);
  }
  return launch_status("ps_chan_layernorm_f32");
}

extern "C" int ps_film_apply_f32(const float* x, const float* scale_bias, float* y, int N, int C, int T, int ldt,
                                 void* stream) {
  if (!x || !scale_bias || !y || N <= 0 || C <= 0 || T <= 0 || ldt < T || C > 65535 || N > 65535) {
    set_error("ps_film_apply_f32: bad argument (N=%d C=%d T=%d ldt=%d)", N, C, T, ldt);
    return PS_E_INVALID;
  }
  if (ldt % 4 || ((uintptr_t)x & 15) || ((uintptr_t)scale_bias & 15) || ((uintptr_t)y & 15)) {
    set_error("ps_film_apply_f32: rows must be 16-byte aligned");
    return PS_E_ALIGN;
  }
  {
    LaunchTimer timer("film_apply", (hipStream_t)stream);
    hipLaunchKernelGGL(film_apply_kernel, dim3((T + 1023) / 1024, C, N), dim3(256), 0, (hipStream_t)stream, x,
                       scale_bias, y, C, T, ldt);
  }
  return launch_status("ps_film_apply_f32");
}

extern "C" int ps_lstm_cell_f32(const float* gates, float* c, float* h, int N, int H, int D, int T, int ld_gates,
                                int ld_state, void* stream) {
  if (!gates || !c || !h || N <= 0 || H <= 0 || D < 1 || D > 2 || T <= 0 || ld_gates < T || ld_state < T ||
      (long long)N * D > 65535) {
    set_error("ps_lstm_cell_f32: bad argument (N=%d H=%d D=%d T=%d)", N, H, D, T);
    return PS_E_INVALID;
  }
  {
    LaunchTimer timer("lstm_cell", (hipStream_t)stream);
    hipLaunchKernelGGL(lstm_cell_kernel, dim3((T + 63) / 64, (H + 3) / 4, N * D), dim3(256), 0, (hipStream_t)stream,
                       gates, c, h, H, T, ld_gates, ld_state);
  }
  return launch_status("ps_lstm_cell_f32");
}

extern "C" int ps_unfold_taps_f32(const float* x, float* y, int N, int K, int T, int ldt, int P, int dilation, int left,
                                  const float* scale, const float* shift, const float* embed, int E, void* stream) {
  return ps_unfold_taps_out_f32(x, y, N, K, T, T, ldt, P, dilation, left, scale, shift, embed, E, stream);
}

extern "C" int ps_unfold_taps_out_f32(const float* x, float* y, int N, int K, int T, int T_out, int ldt, int P,
                                      int dilation, int left, const float* scale, const float* shift,
                                      const float* embed, int E, void* stream) {
  if (!x || !y || N <= 0 || K <= 0 || T <= 0 || T_out < T || ldt < T_out || P <= 0 || dilation <= 0 || left < 0 || E < 0 ||
      (E > 0 && !embed) || ((scale == nullptr) != (shift == nullptr)) || (long long)P * (K + E) > 65535 || N > 65535) {
    set_error("ps_unfold_taps_f32: bad argument (N=%d K=%d T=%d P=%d dilation=%d left=%d E=%d)", N, K, T, P, dilation,
              left, E);
    return PS_E_INVALID;
  }
  {
    LaunchTimer timer("unfold_taps", (hipStream_t)stream);
    hipLaunchKernelGGL(unfold_taps_kernel, dim3((T_out + 255) / 256, P * (K + E), N), dim3(256), 0, (hipStream_t)stream,
                       x, y, scale, shift, embed, K, E, T, T_out, ldt, P, dilation, left);
  }
  return launch_status("ps_unfold_taps_f32");
}

static int check_gate_prologue(const ps_prologue& p, const char* side) {
  if (p.norm != PS_NORM_NONE && (!p.gamma || !p.beta)) {
    set_error("ps_gated_product_f32: %s norm needs gamma/beta", side);
    return PS_E_INVALID;
  }
  if (p.norm == PS_NORM_GLOBAL && (!p.stats || p.parts <= 0 || p.count <= 0)) {
    set_error("ps_gated_product_f32: %s PS_NORM_GLOBAL needs stats/parts/count", side);
    return PS_E_INVALID;
  }
  if (p.prelu && !p.slope) {
    set_error("ps_gated_product_f32: %s prelu needs slope", side);
    return PS_E_INVALID;
  }
  return 0;
}

extern "C" int ps_gated_product_f32(const float* left, const float* right, float* y, int N, int H, int T, int ldt,
                                    const ps_prologue* pro_left, const ps_prologue* pro_right, void* stream) {
  if (!left || !right || !y || !pro_left || !pro_right || N <= 0 || H <= 0 || T <= 0 || ldt < T || H > 65535 ||
      N > 65535) {
    set_error("ps_gated_product_f32: bad argument (N=%d H=%d T=%d ldt=%d)", N, H, T, ldt);
    return PS_E_INVALID;
  }
  if (ldt % 4 || ((uintptr_t)left & 15) || ((uintptr_t)right & 15) || ((uintptr_t)y & 15)) {
    set_error("ps_gated_product_f32: rows must be 16-byte aligned");
    return PS_E_ALIGN;
  }
  int rc = check_gate_prologue(*pro_left, "left");
  if (rc) return rc;
  rc = check_gate_prologue(*pro_right, "right");
  if (rc) return rc;
  GateArgs a{left, right, y, *pro_left, *pro_right, H, T, ldt};
  {
    LaunchTimer timer("gated_product", (hipStream_t)stream);
    hipLaunchKernelGGL(gated_product_kernel, dim3((T + 1023) / 1024, H, N), dim3(256), 0, (hipStream_t)stream, a);
  }
  return launch_status("ps_gated_product_f32");
}

extern "C" int ps_segment_overlap_f32(const float* src, float* dst, int64_t rows, int T_src, int ld_src, int T_dst,
                                      int ld_dst, int K, int merge, void* stream) {
  if (!src || !dst || rows <= 0 || rows > 65535 * 32768LL || T_src <= 0 || T_dst <= 0 || ld_src < T_src ||
      ld_dst < T_dst || K < 2) {
    set_error("ps_segment_overlap_f32: bad argument");
    return PS_E_INVALID;
  }
  const int stride = K / 2;
  if (!merge) {
    // every source index the split reads is checked in the kernel; the destination must be whole segment pairs
    if (T_dst % (2 * K)) {
      set_error("ps_segment_overlap_f32: split destination must hold an even number of %d-frame segments", K);
      return PS_E_INVALID;
    }
  } else {
    // the last merged frame reads even-stream index stride + T_dst - 1 and odd-stream index T_dst - 1
    const long long e = (long long)stride + T_dst - 1;
    const long long fa = (2 * (e / K)) * K + e % K, fb = (2LL * ((T_dst - 1) / K) + 1) * K + (T_dst - 1) % K;
    if (fa >= T_src || fb >= T_src) {
      set_error("ps_segment_overlap_f32: merge source is too short (%d frames)", T_src);
      return PS_E_INVALID;
    }
  }
  LaunchTimer timer("segment_overlap", (hipStream_t)stream);
  const int64_t chunk = 65535;
  for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
    const int64_t nr = rows - r0 < chunk ? rows - r0 : chunk;
    hipLaunchKernelGGL(segment_overlap_kernel, dim3((T_dst + 255) / 256, (unsigned)nr), dim3(256), 0,
                       (hipStream_t)stream, src + r0 * ld_src, dst + r0 * ld_dst, T_src, ld_src, T_dst, ld_dst, K, merge);
  }
  return launch_status("ps_segment_overlap_f32");
}
