// k causal frames of the time-domain Conv-TasNet (FreeEncDec + causal ConvTasNet, egs/tse td_tse_conv_tasnet_v0_causal) for
// B concurrent streams (puresound_amd/streaming/tcn.py).  As in stream_step.hip the streams are the column axis of the
// library's channel-major rows: k frames of B streams are the N = k * B columns of one [1][C][ld] tensor, column f * B + b =
// frame f of the chunk, stream b, so the 1x1 convolutions are ps_conv1x1_f32 with N columns.  What needs earlier frames
// lives in per-stream state here: a history ring per depthwise convolution, an overlap-add tail for the decoder, and the
// device frame counter (absolute index of the chunk's first frame) that no launch argument depends on.
//
// ps_dwconv_step_f32       causal depthwise dilated convolution over the chunk's k frames, taps before the chunk from a ring
// ps_free_decode_step_f32  mask x features, the [win x C] synthesis product and the overlap-add of k frames per stream
//
// Slots (ps_dwconv_step_slots_f32, ps_free_decode_step_slots_f32): the same two with a per-stream span [B][2] of absolute
// frame indices.  Frame g of stream b is live iff span[b][0] <= g < span[b][1]; a frame that is not live is read as 0 by
// every depthwise tap and adds nothing to the overlap-add, so a column can begin and end a stream of its own while the
// session runs.  The gate is a compile-time variant of the kernel bodies (template <bool SLOTS>): the kernels the entry
// points without a span launch are the code they were.
#include "ps_common.h"

namespace ps {

// ---------------------------------------------------------------------------------------------------------------------
// ps_dwconv_step_f32.  One thread per (channel h, column n = f * B + b):
//   y[h][n] = bias[h] + sum_j w[h][j] * a(t0 + f - (P-1-j) * d),  t0 = *counter,
// a(g) = PReLU(affine(x)) of the chunk's own column when g >= t0, ring slot g % R (activated values) when 0 <= g < t0, and 0
// when g < 0 -- the causal zero padding is decided from the counter, so it is a zero AFTER the prologue, as ps_dwconv_f32
// pads.  The thread then stores its own activated value in slot (t0 + f) % R.  R >= (P-1) * d + k: a slot written here
// holds a frame at least R frames newer than any the other taps of this launch read from that slot, so no read sees a
// write of the same launch.  The ring is circular: a hop moves (k + P) * H * B values, whatever R is.
// ---------------------------------------------------------------------------------------------------------------------
struct DwStepArgs {
  const float* x;
  float* ring;
  const int* counter;
  const float* w;
  const float* b;
  float* y;
  ps_prologue pro;
  int H, B, k, ld, P, dilation, R;
};

__device__ __forceinline__ float dw_step_act(float v, float sc, float sh, bool norm, bool prelu, float slope) {
  float z = norm ? v * sc + sh : v;
  if (prelu) z = (slope >= 0.f && slope <= 1.f) ? fmaxf(z, slope * z) : ps::prelu(z, slope);
  return z;
}

// SLOTS: "frame g exists" is span[b][0] <= g < span[b][1] instead of g >= 0, for the chunk's own columns as for the ring.
// A slot of the ring that a dead frame owns may hold anything (the thread stores its own activated value whether its frame
// is live or not, and nothing clears the ring when a stream begins): every read is gated, and the gate selects an exact 0.
template <bool SLOTS>
__device__ __forceinline__ void dwconv_step_body(const DwStepArgs& a, const int* __restrict__ span) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int h = blockIdx.y;
  const int N = a.k * a.B;
  if (n >= N) return;
  const int f = n / a.B, b = n - f * a.B;
  const int t0 = *a.counter;
  int lo = 0, hi = 0;
  if constexpr (SLOTS) {
    const int2 sp = reinterpret_cast<const int2*>(span)[b];
    lo = sp.x > 0 ? sp.x : 0;   // (a ring slot index is never taken from a negative frame)
    hi = sp.y;
  }
  const bool norm = a.pro.norm == PS_NORM_AFFINE;
  const bool prelu = a.pro.prelu != 0;
  const float sc = norm ? a.pro.gamma[h] : 1.f, sh = norm ? a.pro.beta[h] : 0.f;
  const float slope = prelu ? a.pro.slope[0] : 1.f;
  const float* xr = a.x + (size_t)h * a.ld;
  const size_t slab = (size_t)a.H * a.B;  // one ring slot: [H][B]
  float acc = a.b ? a.b[h] : 0.f;
  float own = 0.f;
  for (int j = 0; j < a.P; ++j) {
    const int fs = f - (a.P - 1 - j) * a.dilation;
    float v;
    if (fs >= 0) {
      v = dw_step_act(xr[(size_t)fs * a.B + b], sc, sh, norm, prelu, slope);
      if (fs == f) own = v;
      if constexpr (SLOTS) {
        const int g = t0 + fs;
        v = (g >= lo && g < hi) ? v : 0.f;
      }
    } else {
      const int g = t0 + fs;
      if constexpr (SLOTS)
        v = (g >= lo && g < hi) ? a.ring[(size_t)(g % a.R) * slab + (size_t)h * a.B + b] : 0.f;
      else
        v = g >= 0 ? a.ring[(size_t)(g % a.R) * slab + (size_t)h * a.B + b] : 0.f;
    }
    acc += a.w[h * a.P + j] * v;
  }
  a.y[(size_t)h * a.ld + n] = acc;
  a.ring[(size_t)((t0 + f) % a.R) * slab + (size_t)h * a.B + b] = own;
}

__global__ __launch_bounds__(256) void dwconv_step_kernel(DwStepArgs a) { dwconv_step_body<false>(a, nullptr); }

__global__ __launch_bounds__(256) void dwconv_step_slots_kernel(DwStepArgs a, const int* __restrict__ span) {
  dwconv_step_body<true>(a, span);
}

// ---------------------------------------------------------------------------------------------------------------------
// ps_free_decode_step_f32, two launches.
// Synthesis: s[f][j][b] = sum_c w[c][j] feats[c][f B + b] act(mask[c][f B + b]) into the workspace [k][win][B].  One
// workgroup per (64 streams, frame f, 16 taps): 256 threads = 64 streams x 4 groups of 4 taps, every thread walks the C
// channels for its stream (coalesced over the streams; the weight addresses are uniform across a wave).
// Overlap-add: thread (r, b), r < hop, owns the samples r + m hop of stream b, m = 0 .. k + win/hop - 2, in increasing m:
// v = tail[b][r + m hop] (m < win/hop - 1) + s[f][r + m hop - f hop][b] over the frames f <= m that cover the sample, in
// increasing f; m < k: out[b][r + m hop] = constrain(v); m >= k: tail[b][r + (m-k) hop] = v.  The tail slot the thread
// writes at step m it read at step m - k, and no other thread touches it.  flush: out = constrain(tail).
// SLOTS: the synthesis of a frame g = *counter + f outside span[b] stores 0 and reads nothing (the column may hold inf / NaN:
// an idle slot's input is whatever the caller passed), so the overlap-add, which is the same kernel, adds nothing for it.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int DEC_SB = 64;   // streams per workgroup
constexpr int DEC_JW = 16;   // taps per workgroup: 4 groups x 4

__device__ __forceinline__ float dec_mask_act(float m, int act) {
  if (act == PS_ACT_RELU) return relu_keep_nan(m);
  if (act == PS_ACT_SIGMOID) return 1.f / (1.f + expf(-m));
  return m;
}

__device__ __forceinline__ float dec_constrain(float v, int mode) {
  if (mode == PS_OUT_CLAMP) return clamp1_keep_nan(v);
  if (mode == PS_OUT_SIGMOID) return 1.f / (1.f + expf(-v));
  return v;
}

// Extra: nothing, or (const int* span, const int* counter) when SLOTS -- a trailing pack, so that the instantiation without
// slots keeps the argument list (and with it the code) the kernel had before there were slots.
template <bool SLOTS, typename... Extra>
__global__ __launch_bounds__(256) void free_decode_synth_kernel(const float* __restrict__ feats, const float* __restrict__ mask,
                                                                int mask_mode, int ld, const float* __restrict__ w,
                                                                float* __restrict__ syn, int B, int C, int win,
                                                                Extra... extra) {
  static_assert(sizeof...(Extra) == (SLOTS ? 2 : 0), "SLOTS: span and counter");
  const int tid = threadIdx.x;
  const int b = blockIdx.x * DEC_SB + tid % DEC_SB;
  const int f = blockIdx.y;
  const int j0 = blockIdx.z * DEC_JW + __builtin_amdgcn_readfirstlane(tid / DEC_SB) * 4;  // (uniform across the wave)
  if (b >= B) return;
  if constexpr (SLOTS) {
    const int* const ex[] = {extra...};   // span [B][2], counter
    const int2 sp = reinterpret_cast<const int2*>(ex[0])[b];
    const int g = *ex[1] + f;
    if (g < sp.x || g >= sp.y) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j0 + u < win) syn[((size_t)f * win + j0 + u) * B + b] = 0.f;
      return;
    }
  }
  const size_t col = (size_t)f * B + b;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int c = 0;
  for (; c + 4 <= C; c += 4) {
    float e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) e[q] = feats[(size_t)(c + q) * ld + col];
    if (mask) {
#pragma unroll
      for (int q = 0; q < 4; ++q) e[q] *= dec_mask_act(mask[(size_t)(c + q) * ld + col], mask_mode);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* wc = w + (size_t)(c + q) * win;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j0 + u < win) acc[u] = fmaf(wc[j0 + u], e[q], acc[u]);
    }
  }
  for (; c < C; ++c) {
    float e = feats[(size_t)c * ld + col];
    if (mask) e *= dec_mask_act(mask[(size_t)c * ld + col], mask_mode);
    const float* wc = w + (size_t)c * win;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (j0 + u < win) acc[u] = fmaf(wc[j0 + u], e, acc[u]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (j0 + u < win) syn[((size_t)f * win + j0 + u) * B + b] = acc[u];
}

__global__ __launch_bounds__(256) void free_decode_ola_kernel(const float* __restrict__ syn, float* __restrict__ tail,
                                                              float* __restrict__ out, int ld_out, int B, int k, int win,
                                                              int hop, int out_mode) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * hop) return;
  const int r = i / B, b = i - r * B;
  const int R = win / hop, keep = win - hop;
  for (int m = 0; m < k + R - 1; ++m) {
    const int s = r + m * hop;
    float v = m < R - 1 ? tail[(size_t)b * keep + s] : 0.f;
    const int f_lo = m - R + 1 > 0 ? m - R + 1 : 0, f_hi = m < k - 1 ? m : k - 1;
    for (int f = f_lo; f <= f_hi; ++f) v += syn[((size_t)f * win + (s - f * hop)) * B + b];
    if (m < k)
      out[(size_t)b * ld_out + s] = dec_constrain(v, out_mode);
    else
      tail[(size_t)b * keep + (s - k * hop)] = v;
  }
}

__global__ __launch_bounds__(256) void free_decode_flush_kernel(const float* __restrict__ tail, float* __restrict__ out,
                                                                int ld_out, int B, int keep, int out_mode) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * keep) return;
  const int b = i / keep, s = i - b * keep;
  out[(size_t)b * ld_out + s] = dec_constrain(tail[i], out_mode);
}

}  // namespace ps

using namespace ps;

// ps_dwconv_step_f32 (span = NULL, slots = false) and ps_dwconv_step_slots_f32 share the checks and differ in the kernel.
static int dwconv_step_launch(const char* who, bool slots, const float* x, float* ring, int R, const int* counter,
                              const int* span, const float* w, const float* b, float* y, int H, int B, int k, int ld, int P,
                              int dilation, const ps_prologue* pro, void* stream) {
  if (!x || !ring || !counter || !w || !y || H <= 0 || H > 65535 || B <= 0 || k <= 0 || P <= 0 || dilation <= 0 ||
      (long long)k * B > ld || (long long)H * ld > (1LL << 31) || (long long)R * H * B > (1LL << 40) || x == y) {
    set_error("%s: bad argument (H=%d B=%d k=%d ld=%d P=%d dilation=%d R=%d)", who, H, B, k, ld, P, dilation, R);
    return PS_E_INVALID;
  }
  if (slots && (!span || ((uintptr_t)span & 7))) {
    set_error("%s: span must be an 8-byte aligned device array [B][2] of int", who);
    return PS_E_INVALID;
  }
  if ((long long)R < (long long)(P - 1) * dilation + k) {
    set_error("%s: the ring holds %d frames; (P-1)*dilation + k = %lld needed", who, R, (long long)(P - 1) * dilation + k);
    return PS_E_INVALID;
  }
  DwStepArgs a{x, ring, counter, w, b, y, ps_prologue{}, H, B, k, ld, P, dilation, R};
  if (pro) {
    if (pro->norm != PS_NORM_NONE && pro->norm != PS_NORM_AFFINE) {
      set_error("%s: prologue norm %d: none or PS_NORM_AFFINE (a global norm does not stream)", who, pro->norm);
      return PS_E_UNSUPPORTED;
    }
    if ((pro->norm == PS_NORM_AFFINE && (!pro->gamma || !pro->beta)) || (pro->prelu && !pro->slope) || pro->pre_relu ||
        pro->post_tanh) {
      set_error("%s: the affine prologue needs gamma / beta, PReLU a slope; no pre_relu / post_tanh", who);
      return PS_E_INVALID;
    }
    a.pro = *pro;
  }
  const int N = k * B;
  LaunchTimer timer(slots ? "dwconv_step_slots" : "dwconv_step", (hipStream_t)stream);
  if (slots)
    hipLaunchKernelGGL(dwconv_step_slots_kernel, dim3((N + 255) / 256, H), dim3(256), 0, (hipStream_t)stream, a, span);
  else
    hipLaunchKernelGGL(dwconv_step_kernel, dim3((N + 255) / 256, H), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status(who);
}

extern "C" int ps_dwconv_step_f32(const float* x, float* ring, int R, const int* counter, const float* w, const float* b,
                                  float* y, int H, int B, int k, int ld, int P, int dilation, const ps_prologue* pro,
                                  void* stream) {
  return dwconv_step_launch("ps_dwconv_step_f32", false, x, ring, R, counter, nullptr, w, b, y, H, B, k, ld, P, dilation, pro,
                            stream);
}

extern "C" int ps_dwconv_step_slots_f32(const float* x, float* ring, int R, const int* counter, const int* span,
                                        const float* w, const float* b, float* y, int H, int B, int k, int ld, int P,
                                        int dilation, const ps_prologue* pro, void* stream) {
  return dwconv_step_launch("ps_dwconv_step_slots_f32", true, x, ring, R, counter, span, w, b, y, H, B, k, ld, P, dilation,
                            pro, stream);
}

extern "C" size_t ps_free_decode_step_workspace_bytes(int B, int k, int win) {
  if (B <= 0 || k <= 0 || win <= 0) return 0;
  return (size_t)k * win * B * sizeof(float);
}

// span = NULL: ps_free_decode_step_f32; else ps_free_decode_step_slots_f32 (never a flush).
static int free_decode_step_launch(const char* who, const float* feats, const float* mask, int mask_act, int ld,
                                   const float* w, float* tail, float* out, int ld_out, int B, int k, int C, int win, int hop,
                                   int out_mode, int flush, float* ws, size_t ws_bytes, const int* span, const int* counter,
                                   void* stream) {
  const int keep = win - hop;
  if ((!out && !(flush && keep == 0)) || B <= 0 || hop <= 0 || win < hop || win % hop || win > 256 || (keep > 0 && !tail) ||
      (flush != 0 && flush != 1) || out_mode < PS_OUT_CLAMP || out_mode > PS_OUT_NONE ||
      (!flush && (!feats || !w || k <= 0 || k > 65535 || C <= 0 || (long long)k * B > ld || (long long)C * ld > (1LL << 31) ||
                  ld_out < k * hop || mask_act < PS_ACT_LINEAR || mask_act > PS_ACT_SIGMOID || !ws ||
                  ws_bytes < ps_free_decode_step_workspace_bytes(B, k, win))) ||
      (flush && ld_out < keep)) {
    set_error("%s: bad argument (B=%d k=%d C=%d win=%d hop=%d ld=%d ld_out=%d flush=%d ws=%zu)", who, B, k, C, win, hop, ld,
              ld_out, flush, ws_bytes);
    return PS_E_INVALID;
  }
  LaunchTimer timer(span ? "free_decode_step_slots" : "free_decode_step", (hipStream_t)stream);
  if (flush) {
    if (keep == 0) return 0;  // win = hop: nothing overlaps the last frame
    hipLaunchKernelGGL(free_decode_flush_kernel, dim3((B * keep + 255) / 256), dim3(256), 0, (hipStream_t)stream, tail, out,
                       ld_out, B, keep, out_mode);
    return launch_status(who);
  }
  const dim3 grid((B + DEC_SB - 1) / DEC_SB, k, (win + DEC_JW - 1) / DEC_JW);
  if (span)
    hipLaunchKernelGGL((free_decode_synth_kernel<true, const int*, const int*>), grid, dim3(256), 0, (hipStream_t)stream, feats, mask, mask_act, ld, w,
                       ws, B, C, win, span, counter);
  else
    hipLaunchKernelGGL((free_decode_synth_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, feats, mask, mask_act, ld, w, ws, B,
                       C, win);
  hipLaunchKernelGGL(free_decode_ola_kernel, dim3((B * hop + 255) / 256), dim3(256), 0, (hipStream_t)stream, ws, tail, out,
                     ld_out, B, k, win, hop, out_mode);
  return launch_status(who);
}

extern "C" int ps_free_decode_step_f32(const float* feats, const float* mask, int mask_act, int ld, const float* w,
                                       float* tail, float* out, int ld_out, int B, int k, int C, int win, int hop,
                                       int out_mode, int flush, float* ws, size_t ws_bytes, void* stream) {
  return free_decode_step_launch("ps_free_decode_step_f32", feats, mask, mask_act, ld, w, tail, out, ld_out, B, k, C, win, hop,
                                 out_mode, flush, ws, ws_bytes, nullptr, nullptr, stream);
}

extern "C" int ps_free_decode_step_slots_f32(const float* feats, const float* mask, int mask_act, int ld, const float* w,
                                             float* tail, float* out, int ld_out, const int* span, const int* counter, int B,
                                             int k, int C, int win, int hop, int out_mode, float* ws, size_t ws_bytes,
                                             void* stream) {
  if (!span || ((uintptr_t)span & 7) || !counter) {
    set_error("ps_free_decode_step_slots_f32: span (8-byte aligned device int [B][2]) and counter (device int) are required");
    return PS_E_INVALID;
  }
  return free_decode_step_launch("ps_free_decode_step_slots_f32", feats, mask, mask_act, ld, w, tail, out, ld_out, B, k, C,
                                 win, hop, out_mode, 0, ws, ws_bytes, span, counter, stream);
}
