// k causal frames of ONE block of the causal dual-path RNN (DPRNN, causal=True, seg_overlap=False) for B concurrent streams in
// one launch (puresound_amd/streaming/dprnn.py).  Layout as tcn_step.hip: the k frames of a chunk for the B streams are the
// columns f * B + b of a [1][C][ld] tensor, and `counter` is the device frame counter (absolute index of the chunk's first
// frame), which the kernel reads and never writes, so no launch argument depends on the frame index.
//
// Frame g = *counter + f sits at position p = g % K of its segment.  Per frame and column:
//   intra:  (h, c) = (h_intra, c_intra), read as 0 when p == 0 (every segment starts the intra LSTM from zero);
//           gates = W [x ; h] + b, LSTM cell (gates i, f, g, o), y = x + LN(P h' + b_p); (h', c') -> (h_intra, c_intra)
//   inter:  the same on y with (h, c) = slot p of the banks [K][H][ldb] (the state the previous segment left at position p),
//           written back to slot p; out = y + LN(P h'' + b_p)
// Every dependency is per stream, so a workgroup owns DP_TB stream columns, walks the chunk's frames in order and never
// reads another workgroup's columns or state: one launch per block, and a stream's values cannot depend on its neighbours.
//
// Work inside a workgroup (256 threads, 16 columns): the gate product gives one gate row to a thread for all 16 columns
// (the weight, stored k-major, is read once per workgroup, coalesced over the rows, from L2; the 16 inputs of a k are a
// broadcast read of LDS); the cell runs on (unit, column) pairs; the projection gives a thread one output row and 8 columns;
// LayerNorm gives a column to 16 lanes, which sum strided partials and combine them by a butterfly.  Every sum of a column
// has one fixed order (k ascending with fmaf from the bias; the LN partials by lane, then xor 8, 4, 2, 1), so a stream's bits
// do not depend on B, on its neighbours or on how the hops are split into chunks.  A state element is loaded and stored by
// the same thread, so a bank slot revisited within a chunk (k > K) is read back by the thread that wrote it.
//
// Slots (ps_dprnn_block_step_slots_f32): the same with a per-stream span [B][2] of absolute frame indices, as tcn_step.hip.
// Column b is live at frame g iff span[b][0] <= g < span[b][1], and a live column has a phase of its own: its position is
// p_b = (g - span[b][0]) % K, so the intra reset (p_b == 0) and the bank slot (p_b) differ between the columns of a tile.
// Every loop that touches state, x or y strides by 256 over an index whose column is i % 16, so a thread only ever serves
// column tid % 16: it reads that column's span once per launch and keeps liveness and p_b in registers.  A dead column reads
// x and its states as 0 (it may hold inf / NaN) and stores no state; its y is written, finite.  The 16 columns sit in lanes
// 16 q .. 16 q + 15 of every wave, so a wave's vote "any column live" is the same in every wave of the workgroup: a frame at
// which the whole tile is dead skips both passes (no barrier is passed by some waves only) and stores y = 0.  The gate is a
// compile-time variant (template <bool SLOTS>): the kernel the entry point without a span launches is the code it was.
#include "ps_common.h"

namespace ps {

constexpr int DP_TB = 16;        // stream columns per workgroup
constexpr int DP_THREADS = 256;

struct DprnnStepArgs {
  const float* x;
  float* y;
  const int* counter;
  ps_dprnn_pass intra, inter;
  float *h_intra, *c_intra, *h_bank, *c_bank;
  int C, H, K, B, k, ld, ldb;
};

__device__ __forceinline__ float dp_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// Sum over the 16 lanes that share a column (lanes 16 q .. 16 q + 15 of a wave), the same order in every lane.
__device__ __forceinline__ float dp_sum16(float v) {
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}

// One LSTM + projection + LayerNorm + residual pass on the tile: xh rows [0, C) hold the input and receive the output,
// rows [C, C + H) and cs are scratch for (h, c); hs / cs_g point at the state rows [H][ldb] of column b0.
// SLOTS: hs / cs_g, from_zero and alive are this thread's column's (column tid % 16): its bank slot, its segment start,
// whether its frame is live (a column past `cols` is never alive).
template <bool SLOTS>
__device__ __forceinline__ void dprnn_pass(const ps_dprnn_pass& w, float* xh, float* cs, float* gt, float* pr, float* hs,
                                           float* cs_g, bool from_zero, bool alive, int C, int H, int ldb, int cols) {
  const int tid = threadIdx.x;
  const int G = 4 * H, KK = C + H;
  for (int i = tid; i < H * DP_TB; i += DP_THREADS) {
    const int u = i / DP_TB, j = i % DP_TB;
    bool live = j < cols && !from_zero;
    if constexpr (SLOTS) live = alive && !from_zero;
    xh[(C + u) * DP_TB + j] = live ? hs[(size_t)u * ldb + j] : 0.f;
    cs[i] = live ? cs_g[(size_t)u * ldb + j] : 0.f;
  }
  __syncthreads();
  for (int r = tid; r < G; r += DP_THREADS) {
    float acc[DP_TB];
    const float b = w.bias[r];
#pragma unroll
    for (int j = 0; j < DP_TB; ++j) acc[j] = b;
    const float* wr = w.wt + r;
#pragma unroll 4
    for (int k = 0; k < KK; ++k) {
      const float wk = wr[(size_t)k * G];
      const float4* xv = reinterpret_cast<const float4*>(xh + k * DP_TB);
#pragma unroll
      for (int q = 0; q < DP_TB / 4; ++q) {
        const float4 v = xv[q];
        acc[4 * q + 0] = fmaf(wk, v.x, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(wk, v.y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(wk, v.z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(wk, v.w, acc[4 * q + 3]);
      }
    }
    float4* go = reinterpret_cast<float4*>(gt + r * DP_TB);
#pragma unroll
    for (int q = 0; q < DP_TB / 4; ++q) go[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
  }
  __syncthreads();
  for (int i = tid; i < H * DP_TB; i += DP_THREADS) {
    const int u = i / DP_TB, j = i % DP_TB;
    const float gi = dp_sigmoid(gt[u * DP_TB + j]);
    const float gf = dp_sigmoid(gt[(H + u) * DP_TB + j]);
    const float gg = tanhf(gt[(2 * H + u) * DP_TB + j]);
    const float go = dp_sigmoid(gt[(3 * H + u) * DP_TB + j]);
    const float cn = gf * cs[i] + gi * gg;
    const float hn = go * tanhf(cn);
    xh[(C + u) * DP_TB + j] = hn;
    bool store = j < cols;
    if constexpr (SLOTS) store = alive;
    if (store) {
      hs[(size_t)u * ldb + j] = hn;
      cs_g[(size_t)u * ldb + j] = cn;
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * C; i += DP_THREADS) {
    const int m = i % C, half = i / C;
    float acc[8];
    const float b = w.pbias[m];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = b;
    const float* pm = w.pt + m;
    const float* hv = xh + C * DP_TB + half * 8;
#pragma unroll 4
    for (int k = 0; k < H; ++k) {
      const float wk = pm[(size_t)k * C];
      const float4 v0 = *reinterpret_cast<const float4*>(hv + k * DP_TB);
      const float4 v1 = *reinterpret_cast<const float4*>(hv + k * DP_TB + 4);
      acc[0] = fmaf(wk, v0.x, acc[0]);
      acc[1] = fmaf(wk, v0.y, acc[1]);
      acc[2] = fmaf(wk, v0.z, acc[2]);
      acc[3] = fmaf(wk, v0.w, acc[3]);
      acc[4] = fmaf(wk, v1.x, acc[4]);
      acc[5] = fmaf(wk, v1.y, acc[5]);
      acc[6] = fmaf(wk, v1.z, acc[6]);
      acc[7] = fmaf(wk, v1.w, acc[7]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) pr[m * DP_TB + half * 8 + j] = acc[j];
  }
  __syncthreads();
  {
    const int col = tid / 16, l = tid % 16;   // 256 threads = 16 columns x 16 lanes
    float s = 0.f;
    for (int m = l; m < C; m += 16) s += pr[m * DP_TB + col];
    const float mean = dp_sum16(s) / (float)C;
    float q = 0.f;
    for (int m = l; m < C; m += 16) {
      const float d = pr[m * DP_TB + col] - mean;
      q = fmaf(d, d, q);
    }
    const float rstd = 1.f / sqrtf(dp_sum16(q) / (float)C + w.eps);
    for (int m = l; m < C; m += 16)
      xh[m * DP_TB + col] += (pr[m * DP_TB + col] - mean) * rstd * w.gamma[m] + w.beta[m];
  }
  __syncthreads();
}

template <bool SLOTS>
__device__ __forceinline__ void dprnn_block_step_body(const DprnnStepArgs& a, const int* __restrict__ span) {
  extern __shared__ __align__(16) float dp_lds[];
  const int C = a.C, H = a.H;
  float* xh = dp_lds;                        // [C + H][16]
  float* cs = xh + (C + H) * DP_TB;          // [H][16]
  float* gt = cs + H * DP_TB;                // [4H][16]
  float* pr = gt + 4 * H * DP_TB;            // [C][16]
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * DP_TB;
  const int cols = a.B - b0 < DP_TB ? a.B - b0 : DP_TB;
  const int t0 = *a.counter;
  const size_t slab = (size_t)H * a.ldb;     // one bank slot
  int lo = 0, hi = 0;                        // this thread's column's span (empty past the last stream)
  if constexpr (SLOTS) {
    if (tid % DP_TB < cols) {
      const int2 sp = reinterpret_cast<const int2*>(span)[b0 + tid % DP_TB];
      lo = sp.x;
      hi = sp.y;
    }
  }
  for (int f = 0; f < a.k; ++f) {
    const size_t c0 = (size_t)f * a.B + b0;
    if constexpr (SLOTS) {
      const int g = t0 + f;
      const bool alive = g >= lo && g < hi;
      if (!__any(alive)) {                   // the whole tile is dead at this frame (the same vote in every wave)
        for (int i = tid; i < C * DP_TB; i += DP_THREADS) {
          const int m = i / DP_TB, j = i % DP_TB;
          if (j < cols) a.y[(size_t)m * a.ld + c0 + j] = 0.f;
        }
        continue;
      }
      const int p = alive ? (int)(((unsigned)g - (unsigned)lo) % (unsigned)a.K) : 0;   // (g - lo < 2^32: exact)
      for (int i = tid; i < C * DP_TB; i += DP_THREADS) {
        const int m = i / DP_TB, j = i % DP_TB;
        xh[i] = alive ? a.x[(size_t)m * a.ld + c0 + j] : 0.f;
      }
      dprnn_pass<true>(a.intra, xh, cs, gt, pr, a.h_intra + b0, a.c_intra + b0, p == 0, alive, C, H, a.ldb, cols);
      dprnn_pass<true>(a.inter, xh, cs, gt, pr, a.h_bank + p * slab + b0, a.c_bank + p * slab + b0, false, alive, C, H,
                       a.ldb, cols);
    } else {
      const int p = (t0 + f) % a.K;
      for (int i = tid; i < C * DP_TB; i += DP_THREADS) {
        const int m = i / DP_TB, j = i % DP_TB;
        xh[i] = j < cols ? a.x[(size_t)m * a.ld + c0 + j] : 0.f;
      }
      // (the pass's first barrier also covers these stores)
      dprnn_pass<false>(a.intra, xh, cs, gt, pr, a.h_intra + b0, a.c_intra + b0, p == 0, true, C, H, a.ldb, cols);
      dprnn_pass<false>(a.inter, xh, cs, gt, pr, a.h_bank + p * slab + b0, a.c_bank + p * slab + b0, false, true, C, H,
                        a.ldb, cols);
    }
    for (int i = tid; i < C * DP_TB; i += DP_THREADS) {   // (the thread that stores xh[i] for the next frame reads it here)
      const int m = i / DP_TB, j = i % DP_TB;
      if (j < cols) a.y[(size_t)m * a.ld + c0 + j] = xh[i];
    }
  }
}

__global__ __launch_bounds__(DP_THREADS) void dprnn_block_step_kernel(DprnnStepArgs a) {
  dprnn_block_step_body<false>(a, nullptr);
}

// (at most 4 waves per SIMD, the sibling's occupancy -- LDS allows no more at the preset's shape: with a fifth in sight the
// scheduler keeps the slot variant under 96 VGPRs by waiting for each weight load of the projection loop in turn)
__global__ __launch_bounds__(DP_THREADS) __attribute__((amdgpu_waves_per_eu(1, 4))) void dprnn_block_step_slots_kernel(DprnnStepArgs a, const int* __restrict__ span) {
  dprnn_block_step_body<true>(a, span);
}

static size_t dprnn_lds_bytes(int C, int H) { return (size_t)(2 * C + 6 * H) * DP_TB * sizeof(float); }

}  // namespace ps

using namespace ps;

extern "C" int ps_dprnn_block_step_ok(int C, int H, int K) {
  if (C < 1 || H < 1 || K < 1) return PS_E_UNSUPPORTED;
  return dprnn_lds_bytes(C < 4096 ? C : 4096, H < 4096 ? H : 4096) <= 64 * 1024 ? 1 : PS_E_UNSUPPORTED;
}

// ps_dprnn_block_step_f32 (span = NULL, slots = false) and ps_dprnn_block_step_slots_f32 share the checks and differ in the
// kernel.
static int dprnn_block_step_launch(const char* who, bool slots, const float* x, float* y, const int* counter, const int* span,
                                   const ps_dprnn_pass* intra, const ps_dprnn_pass* inter, float* h_intra, float* c_intra,
                                   float* h_bank, float* c_bank, int C, int H, int K, int B, int k, int ld, int ldb,
                                   void* stream) {
  if (!x || !y || x == y || !counter || !intra || !inter || !h_intra || !c_intra || !h_bank || !c_bank || C <= 0 || H <= 0 ||
      K <= 0 || B <= 0 || k <= 0 || ldb < B || (long long)k * B > ld || (long long)C * ld > (1LL << 31) ||
      (long long)K * H * ldb > (1LL << 40)) {
    set_error("%s: bad argument (C=%d H=%d K=%d B=%d k=%d ld=%d ldb=%d)", who, C, H, K, B, k, ld, ldb);
    return PS_E_INVALID;
  }
  if (slots && (!span || ((uintptr_t)span & 7))) {
    set_error("%s: span must be an 8-byte aligned device array [B][2] of int", who);
    return PS_E_INVALID;
  }
  for (const ps_dprnn_pass* w : {intra, inter})
    if (!w->wt || !w->bias || !w->pt || !w->pbias || !w->gamma || !w->beta) {
      set_error("%s: a pass needs wt, bias, pt, pbias, gamma and beta", who);
      return PS_E_INVALID;
    }
  if (ps_dprnn_block_step_ok(C, H, K) != 1) {
    set_error("%s: (C, H, K) = (%d, %d, %d): the tile of 16 columns needs (2 C + 6 H) * 64 bytes of LDS, 64 KiB at most", who,
              C, H, K);
    return PS_E_UNSUPPORTED;
  }
  DprnnStepArgs a{x, y, counter, *intra, *inter, h_intra, c_intra, h_bank, c_bank, C, H, K, B, k, ld, ldb};
  LaunchTimer timer(slots ? "dprnn_block_step_slots" : "dprnn_block_step", (hipStream_t)stream);
  if (slots)
    hipLaunchKernelGGL(dprnn_block_step_slots_kernel, dim3((B + DP_TB - 1) / DP_TB), dim3(DP_THREADS), dprnn_lds_bytes(C, H),
                       (hipStream_t)stream, a, span);
  else
    hipLaunchKernelGGL(dprnn_block_step_kernel, dim3((B + DP_TB - 1) / DP_TB), dim3(DP_THREADS), dprnn_lds_bytes(C, H),
                       (hipStream_t)stream, a);
  return launch_status(who);
}

extern "C" int ps_dprnn_block_step_f32(const float* x, float* y, const int* counter, const ps_dprnn_pass* intra,
                                       const ps_dprnn_pass* inter, float* h_intra, float* c_intra, float* h_bank,
                                       float* c_bank, int C, int H, int K, int B, int k, int ld, int ldb, void* stream) {
  return dprnn_block_step_launch("ps_dprnn_block_step_f32", false, x, y, counter, nullptr, intra, inter, h_intra, c_intra,
                                 h_bank, c_bank, C, H, K, B, k, ld, ldb, stream);
}

extern "C" int ps_dprnn_block_step_slots_f32(const float* x, float* y, const int* counter, const int* span,
                                             const ps_dprnn_pass* intra, const ps_dprnn_pass* inter, float* h_intra,
                                             float* c_intra, float* h_bank, float* c_bank, int C, int H, int K, int B, int k,
                                             int ld, int ldb, void* stream) {
  return dprnn_block_step_launch("ps_dprnn_block_step_slots_f32", true, x, y, counter, span, intra, inter, h_intra, c_intra,
                                 h_bank, c_bank, C, H, K, B, k, ld, ldb, stream);
}
