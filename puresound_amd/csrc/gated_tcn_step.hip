// k causal frames of the middle of one GatedTCN block (conv_tasnet.py:129-215, causal = True, eval BatchNorm1d) for B
// concurrent streams (puresound_amd/streaming/unet_tcn.py).  Columns as in tcn_step.hip: y, g [H][ld], column f * B + b =
// frame f of the chunk, stream b; `counter` holds the absolute index t0 of the chunk's first frame; one circular ring
// [R][H][B] of earlier frames of y per block.
//
// ps_gated_tcn_step_f32   g = PReLU(aff_l(L)) * sigmoid(PReLU(aff_r(Rt))), L and Rt the two dense dilated convolutions of y
//
// Both convolutions are GEMMs over the same operand, the P tap-shifted copies of y (K = P * H rows: 768 at the preset), so
// one pass over the gathered taps feeds two accumulator sets and the operand is never written out (ps_unfold_taps_f32 does
// that offline).  VALU, exact fp32 products, as ps_conv2d_step_f32: the operand is a gather over the chunk and the ring,
// and a hop has N = k * B columns -- 64 at B = 64, k = 1.  A workgroup of 256 threads owns TM output channels of both sides
// times 64 columns; TM = 16 up to 1024 columns (16 x 1 workgroups at H = 256, N = 64 and 256 from N = 1024 on: the launch is
// latency-bound there, so the short tile that spreads the K loop over more CUs wins), TM = 32 beyond (two rows per thread
// halve the LDS reads per product).  K runs in slices of 64 through LDS (20 KB at TM = 16, 32 KB at TM = 32).  A hop is a
// chain of dependent launches and a launch a chain of slices, so what a slice costs is memory latency: all its global loads
// (16 gathered values and 4 or 8 weights of each side per thread) are issued before the first is used -- with the gather
// behind a branch per tap the launch took 125 us at the preset's B = 64, with the loads batched 62 us.  Every output sums
// its K products in increasing k in one fmaf chain whatever the tile, so a column's value depends neither on k nor on how
// its stream's frames were split into launches.
#include "ps_common.h"

namespace ps {

struct GatedStepArgs {
  const float* y;
  float* ring;
  const int* counter;
  const float* wl;
  const float* wr;
  const float* emb;   // [P][H][B] or NULL
  float* g;
  const float *sc_l, *sh_l, *slope_l, *sc_r, *sh_r, *slope_r;   // NULL: no affine map / no PReLU on that side
  int H, B, k, ld, P, dilation, R, K, Kp;
};

__device__ __forceinline__ float gated_step_act(float v, const float* sc, const float* sh, const float* slope, int h) {
  float z = sc ? v * sc[h] + sh[h] : v;
  if (slope) {
    const float s = slope[0];
    z = (s >= 0.f && s <= 1.f) ? fmaxf(z, s * z) : ps::prelu(z, s);
  }
  return z;
}

constexpr int GT_TN = 64;   // columns per workgroup
constexpr int GT_KC = 64;   // K slice staged in LDS: 12 slices at K = 768, each one round of global loads and two barriers

// SLOTS (ps_gated_tcn_step_slots_f32): "frame g exists" is span[b][0] <= g < span[b][1] instead of g >= 0, for the chunk's
// own columns as for the ring and for the embedding's tap constants.  A ring slot that a dead frame owns may hold anything
// (every frame of the chunk is stored, and nothing clears the ring when a stream begins): every read is gated, and the gate
// selects an exact 0.  The gate is a compile-time variant of the kernel (template <bool SLOTS>): the kernels the entry without
// a span launches are the code they were.
// Extra: nothing, or (const int* span) when SLOTS -- a trailing pack, so that the instantiation without a span has the kernel
// arguments it always had.
template <int TM, bool SLOTS, typename... Extra>
__global__ __launch_bounds__(256) void gated_tcn_step_kernel(GatedStepArgs a, Extra... extra) {
  static_assert(sizeof...(Extra) == (SLOTS ? 1 : 0), "SLOTS: span");
  const int* span = nullptr;
  if constexpr (SLOTS) {
    const int* const ex[] = {extra...};
    span = ex[0];
  }
  constexpr int RM = TM / 16;   // output channels per thread and side
  __shared__ float Wl[GT_KC][TM];
  __shared__ float Wr[GT_KC][TM];
  __shared__ f32x4 Ys[GT_KC][GT_TN / 4];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * GT_TN, m0 = blockIdx.y * TM;
  const int N = a.k * a.B;
  const int t0 = *a.counter;
  const size_t slab = (size_t)a.H * a.B;   // one ring slot: [H][B]

  // the column this thread gathers, decoded once
  const int gn = tid % GT_TN, gk = tid / GT_TN;
  const int ng = n0 + gn;
  const bool nvalid = ng < N;
  const int gf = nvalid ? ng / a.B : 0, gb = nvalid ? ng - gf * a.B : 0;
  int lo = 0, hi = 0;   // SLOTS: the span of the stream this thread gathers
  if constexpr (SLOTS) {
    if (nvalid) {
      const int2 sp = reinterpret_cast<const int2*>(span)[gb];
      lo = sp.x > 0 ? sp.x : 0;   // (a ring slot index is never taken from a negative frame)
      hi = sp.y;
    }
  }

  // weights: a packed tile holds 256 output channels; TM divides 256, so a tile never straddles two of them
  const size_t woff = (size_t)(m0 / 256) * a.Kp * 256 + (m0 % 256);
  const int tn = tid % 16, tm = tid / 16;

  float accl[RM][4], accr[RM][4];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) accl[i][j] = accr[i][j] = 0.f;

  for (int k0 = 0; k0 < a.K; k0 += GT_KC) {
    // every global load of the slice is issued before the first one is used: the addresses are computed without a branch
    // (a tap that reads nothing loads element 0 of y, and a select drops it), so a slice costs one round of memory latency,
    // not one per tap
    constexpr int WPT = GT_KC * TM / 256, GPT = GT_KC / (256 / GT_TN);
    float wlv[WPT], wrv[WPT], yv[GPT];
    bool yok[GPT];
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int i = tid + u * 256, kk = i / TM, m = i - kk * TM;
      const int row = k0 + kk < a.Kp ? k0 + kk : a.Kp - 1;   // (the packed rows K .. Kp and the channels past H are zeros)
      const size_t o = woff + (size_t)row * 256 + m;
      wlv[u] = a.wl[o];
      wrv[u] = a.wr[o];
    }
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
      const int kx = k0 + gk + u * (256 / GT_TN);
      const int j = kx / a.H, c = kx - j * a.H;
      const int fs = gf - (a.P - 1 - j) * a.dilation;
      const int gfr = t0 + fs;
      const bool own = fs >= 0;
      if constexpr (SLOTS)
        yok[u] = nvalid && kx < a.K && gfr >= lo && gfr < hi;
      else
        yok[u] = nvalid && kx < a.K && (own || gfr >= 0);
      const float* src = own ? a.y : a.ring;
      size_t off = own ? (size_t)c * a.ld + (size_t)fs * a.B + gb : (size_t)(gfr % a.R) * slab + (size_t)c * a.B + gb;
      if (!yok[u]) src = a.y, off = 0;
      yv[u] = src[off];
    }
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int i = tid + u * 256, kk = i / TM, m = i - kk * TM;
      const bool in = k0 + kk < a.Kp;
      Wl[kk][m] = in ? wlv[u] : 0.f;
      Wr[kk][m] = in ? wrv[u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < GPT; ++u)
      reinterpret_cast<float*>(&Ys[gk + u * (256 / GT_TN)][0])[gn] = yok[u] ? yv[u] : 0.f;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GT_KC; ++kk) {
      const f32x4 bv = Ys[kk][tn];
#pragma unroll
      for (int i = 0; i < RM; ++i) {
        const float wl = Wl[kk][tm * RM + i], wr = Wr[kk][tm * RM + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          accl[i][j] = fmaf(wl, bv[j], accl[i][j]);
          accr[i][j] = fmaf(wr, bv[j], accr[i][j]);
        }
      }
    }
    __syncthreads();
  }

  // epilogue: the embedding's tap constants (tap j counts iff its frame is >= 0: the embedding rows are zero-padded with
  // the others), both norms, the sigmoid and the product
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    const int h = m0 + tm * RM + i;
    if (h >= a.H) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + 4 * tn + j;
      if (n >= N) continue;
      const int f = n / a.B, b = n - f * a.B;
      float r = accr[i][j];
      if constexpr (SLOTS) {
        if (a.emb) {
          const int2 sp = reinterpret_cast<const int2*>(span)[b];
          const int elo = sp.x > 0 ? sp.x : 0;   // (the gather's gate: no frame below 0 exists, whatever the birth)
          for (int q = 0; q < a.P; ++q) {
            const int fr = t0 + f - (a.P - 1 - q) * a.dilation;
            if (fr >= elo && fr < sp.y) r += a.emb[((size_t)q * a.H + h) * a.B + b];
          }
        }
      } else {
        if (a.emb)
          for (int q = 0; q < a.P; ++q)
            if (t0 + f - (a.P - 1 - q) * a.dilation >= 0) r += a.emb[((size_t)q * a.H + h) * a.B + b];
      }
      const float lv = gated_step_act(accl[i][j], a.sc_l, a.sh_l, a.slope_l, h);
      const float rv = gated_step_act(r, a.sc_r, a.sh_r, a.slope_r, h);
      a.g[(size_t)h * a.ld + n] = lv * (1.f / (1.f + expf(-rv)));
    }
  }

  // the chunk's frames of channels m0 .. m0 + TM go to their ring slots (every (channel, column) has one owner; the slots
  // written are none of those the taps of this launch read, by R >= (P-1) * dilation + k)
  for (int i = tid; i < TM * GT_TN; i += 256) {
    const int c = m0 + i / GT_TN, n = n0 + i % GT_TN;
    if (c >= a.H || n >= N) continue;
    const int f = n / a.B, b = n - f * a.B;
    const int gfr = t0 + f;
    if (gfr >= 0) a.ring[(size_t)(gfr % a.R) * slab + (size_t)c * a.B + b] = a.y[(size_t)c * a.ld + n];
  }
}

}  // namespace ps

using namespace ps;

static int gated_side(const char* who, const char* side, const ps_prologue* pro, const float** sc, const float** sh,
                      const float** slope) {
  *sc = *sh = *slope = nullptr;
  if (!pro) return 0;
  if (pro->norm != PS_NORM_NONE && pro->norm != PS_NORM_AFFINE) {
    set_error("%s: %s norm %d: none or PS_NORM_AFFINE (a global norm does not stream)", who, side, pro->norm);
    return PS_E_UNSUPPORTED;
  }
  if ((pro->norm == PS_NORM_AFFINE && (!pro->gamma || !pro->beta)) || (pro->prelu && !pro->slope) || pro->pre_relu ||
      pro->post_tanh) {
    set_error("%s: the %s affine map needs gamma / beta, PReLU a slope; no pre_relu / post_tanh", who, side);
    return PS_E_INVALID;
  }
  if (pro->norm == PS_NORM_AFFINE) *sc = pro->gamma, *sh = pro->beta;
  if (pro->prelu) *slope = pro->slope;
  return 0;
}

// ps_gated_tcn_step_f32 (span = NULL, slots = false) and ps_gated_tcn_step_slots_f32 share the checks and differ in the kernel.
static int gated_tcn_step_launch(const char* who, bool slots, const float* y, float* ring, int R, const int* counter,
                                 const int* span, const float* wl, const float* wr, const float* emb_taps,
                                 const ps_prologue* pro_left, const ps_prologue* pro_right, float* g, int H, int B, int k, int ld,
                                 int P, int dilation, void* stream) {
  if (!y || !ring || !counter || !wl || !wr || !g || y == g || H <= 0 || B <= 0 || k <= 0 || P <= 0 || dilation <= 0 ||
      (long long)k * B > ld || (long long)H * ld > (1LL << 31) || (long long)P * H > (1 << 24) ||
      (long long)R * H * B > (1LL << 40) || (long long)P * H * B > (1LL << 31)) {
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
  GatedStepArgs a{};
  if (int rc = gated_side(who, "left", pro_left, &a.sc_l, &a.sh_l, &a.slope_l)) return rc;
  if (int rc = gated_side(who, "right", pro_right, &a.sc_r, &a.sh_r, &a.slope_r)) return rc;
  const long long N = (long long)k * B;
  if ((H + 15) / 16 > 65535) {
    set_error("%s: H = %d: at most 16 * 65535 channels (one grid row per 16)", who, H);
    return PS_E_UNSUPPORTED;
  }
  a.y = y, a.ring = ring, a.counter = counter, a.wl = wl, a.wr = wr, a.emb = emb_taps, a.g = g;
  a.H = H, a.B = B, a.k = k, a.ld = ld, a.P = P, a.dilation = dilation, a.R = R;
  a.K = P * H;
  a.Kp = (a.K + 15) / 16 * 16;
  hipStream_t s = (hipStream_t)stream;
  LaunchTimer timer(slots ? "gated_tcn_step_slots" : "gated_tcn_step", s);
  const unsigned gx = (unsigned)((N + GT_TN - 1) / GT_TN);
  if (slots) {
    if (N <= 1024)
      hipLaunchKernelGGL((gated_tcn_step_kernel<16, true, const int*>), dim3(gx, (H + 15) / 16), dim3(256), 0, s, a, span);
    else
      hipLaunchKernelGGL((gated_tcn_step_kernel<32, true, const int*>), dim3(gx, (H + 31) / 32), dim3(256), 0, s, a, span);
  } else if (N <= 1024)
    hipLaunchKernelGGL((gated_tcn_step_kernel<16, false>), dim3(gx, (H + 15) / 16), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((gated_tcn_step_kernel<32, false>), dim3(gx, (H + 31) / 32), dim3(256), 0, s, a);
  return launch_status(who);
}

extern "C" int ps_gated_tcn_step_f32(const float* y, float* ring, int R, const int* counter, const float* wl, const float* wr,
                                     const float* emb_taps, const ps_prologue* pro_left, const ps_prologue* pro_right,
                                     float* g, int H, int B, int k, int ld, int P, int dilation, void* stream) {
  return gated_tcn_step_launch("ps_gated_tcn_step_f32", false, y, ring, R, counter, nullptr, wl, wr, emb_taps, pro_left,
                               pro_right, g, H, B, k, ld, P, dilation, stream);
}

extern "C" int ps_gated_tcn_step_slots_f32(const float* y, float* ring, int R, const int* counter, const int* span,
                                           const float* wl, const float* wr, const float* emb_taps, const ps_prologue* pro_left,
                                           const ps_prologue* pro_right, float* g, int H, int B, int k, int ld, int P,
                                           int dilation, void* stream) {
  return gated_tcn_step_launch("ps_gated_tcn_step_slots_f32", true, y, ring, R, counter, span, wl, wr, emb_taps, pro_left,
                               pro_right, g, H, B, k, ld, P, dilation, stream);
}
