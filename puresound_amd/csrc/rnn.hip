// Recurrences of the recurrent maskers (DPRNN, SkiM, DPCRN / DPARN of mcw519/PureSound) over gate pre-activations that a
// 1x1 conv already produced (W_ih x + b_ih + b_hh); hout on the library's padded channel-major layout [N][D*H][ldt]:
//
//   ps_lstm_f32, ps_lstm_f16x2_f32   a 1-layer nn.LSTM (both directions), gx channel-major; dprnn.py:155-171, skim.py:215-222
//   ps_lstm_rows_f32                 ps_lstm_f32 with a step count per utterance (ragged batches: SkiM's bidirectional Mem-LSTM
//                                    over each row's own segments, the speaker LSTM over each enrolment's own frames)
//   ps_rnn_f32                       nn.RNN (tanh) / nn.GRU the same way; lobe/rnn.py:19-35
//   ps_lstm_fmajor_*                 gx FRAME-MAJOR: H = 128 (lstm_fm.inc; dpcrn.py:34-81), H = 256 / 192 with W_hh streamed from its
//                                    packed image (lstm_fm256.inc) or resident in the registers of several CUs (lstm_coop.inc)
//
// Order: kernels, checks, dispatch, entries.
//
// LSTM recurrence.  One workgroup owns LS = 4 sequences and all 4H gate rows (thread g = gate row).  W_hh^T stays in
// registers (H <= 64) or is streamed from L2 (coalesced [k][g] rows), h_{t-1} is broadcast from LDS, the four gate
// pre-activations of a unit meet in LDS for the cell update.  A sequence is a strided walk through the frame axis
// (frame = q*q_stride + step*step_stride), which covers the intra-segment pass (q = segment, steps = K
// contiguous frames), the inter-segment pass (q = position in segment, steps = S frames K apart) and the
// streaming step (q = stream, steps = 1).  Gate loads are issued LSTM_PF steps ahead.
#include "ps_common.h"

namespace ps {

constexpr int LS = 4;        // sequences per workgroup
constexpr int LSTM_PF = 8;   // gate pre-activation prefetch distance (steps)
constexpr int LSTM_WREG = 64;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

struct LstmK {
  ps_lstm_args a;
};

// ROWS (ps_lstm_rows_f32): utterance n runs s_n = clamp(steps_rows[n], 0, a.steps) steps, not a.steps: s_n stands where
// a.steps stands in the walk of both directions (direction 1 starts at step s_n - 1), in the prefetch ring's guards (a
// pre-activation at a step >= s_n is never loaded) and in front of the final states; the frames of the steps [s_n, a.steps)
// then get exact zeros.  A workgroup holds one utterance, so s_n is uniform.  A compile-time switch (steps_rows is the one
// extra argument): the plain instantiations keep their instructions.
template <bool WREG, bool ROWS = false, typename... Extra>
__global__ __launch_bounds__(WREG ? 256 : 1024) void lstm_kernel(LstmK k, Extra... extra) {
  extern __shared__ float smem[];
  const ps_lstm_args& a = k.a;
  const int H = a.H, G = 4 * H;
  f32x4* hbuf = reinterpret_cast<f32x4*>(smem);          // [H]  current h of the LS sequences
  f32x4* abuf = hbuf + H;                                  // [4H] gate pre-activations
  const int g = threadIdx.x;
  const int q0 = blockIdx.x * LS, n = blockIdx.y, d = blockIdx.z;
  const bool row = g < G;
  const int DH = a.D * H;

  // recurrent weights of gate row g: column g of W_hh^T [H][4H]
  const float* wt = a.whh_t + (size_t)d * H * G + g;
  float w[LSTM_WREG];
  if constexpr (WREG) {
#pragma unroll
    for (int kk = 0; kk < LSTM_WREG; ++kk) w[kk] = (row && kk < H) ? wt[(size_t)kk * G] : 0.f;
  }

  // cell-update role of this thread: unit j of sequence i (threads [0, H*LS))
  const int j = g % H, i = g / H;
  const bool cell = g < H * LS && q0 + i < a.Q;
  float c = 0.f, h = 0.f;
  if (cell && (a.h0 || a.c0)) {
    const int b = n * a.Q + q0 + i - a.state_shift;
    if (b >= 0) {
      const int nn = b / a.Q, qq = b % a.Q;
      const size_t off = ((size_t)nn * DH + d * H + j) * a.ldq + qq;
      if (a.h0) h = a.h0[off];
      if (a.c0) c = a.c0[off];
    }
  }
  if (g < H * LS) reinterpret_cast<float*>(hbuf)[j * LS + i] = (q0 + i < a.Q) ? h : 0.f;

  // gate pre-activation addressing of row g
  const float* grow = a.gx + ((size_t)n * a.D * G + (size_t)d * G + g) * a.ldt;
  float* hrow = a.hout + ((size_t)n * DH + d * H + j) * a.ldt;
  int steps = a.steps;
  if constexpr (ROWS) {
    const int* const ex[] = {extra...};  // steps_rows [N]
    const int sn = ex[0][n];
    steps = sn < 0 ? 0 : (sn < a.steps ? sn : a.steps);
  }
  const bool rev = d == 1;
  float pre[LSTM_PF][LS];
#pragma unroll
  for (int u = 0; u < LSTM_PF; ++u) {
    const int s = u;
    const int ts = rev ? steps - 1 - s : s;
#pragma unroll
    for (int e = 0; e < LS; ++e)
      pre[u][e] = (row && s < steps && q0 + e < a.Q) ? grow[(size_t)(q0 + e) * a.q_stride + (size_t)ts * a.step_stride]
                                                     : 0.f;
  }
  __syncthreads();

  for (int s0 = 0; s0 < steps; s0 += LSTM_PF) {
#pragma unroll
    for (int u = 0; u < LSTM_PF; ++u) {
      const int s = s0 + u;
      if (s < steps) {  // uniform
        f32x4 acc{pre[u][0], pre[u][1], pre[u][2], pre[u][3]};
        {  // refill this ring slot with step s + LSTM_PF
          const int sn = s + LSTM_PF;
          const int ts = rev ? steps - 1 - sn : sn;
#pragma unroll
          for (int e = 0; e < LS; ++e)
            pre[u][e] = (row && sn < steps && q0 + e < a.Q)
                            ? grow[(size_t)(q0 + e) * a.q_stride + (size_t)ts * a.step_stride]
                            : 0.f;
        }
        if constexpr (WREG) {
#pragma unroll
          for (int kk = 0; kk < LSTM_WREG; ++kk) {
            if (kk < H) {
              const f32x4 hv = hbuf[kk];
              acc += w[kk] * hv;
            }
          }
        } else {
          if (row) {
#pragma unroll 8
            for (int kk = 0; kk < H; ++kk) {
              const f32x4 hv = hbuf[kk];
              acc += wt[(size_t)kk * G] * hv;
            }
          }
        }
        if (row) abuf[g] = acc;
        __syncthreads();
        if (g < H * LS) {
          const float* ab = reinterpret_cast<const float*>(abuf);
          const float gi = sigmoidf_(ab[(j)*LS + i]);
          const float gf = sigmoidf_(ab[(H + j) * LS + i]);
          const float gg = tanhf(ab[(2 * H + j) * LS + i]);
          const float go = sigmoidf_(ab[(3 * H + j) * LS + i]);
          c = gf * c + gi * gg;
          h = go * tanhf(c);
          reinterpret_cast<float*>(hbuf)[j * LS + i] = h;
          if (cell) {
            const int ts = rev ? steps - 1 - s : s;
            hrow[(size_t)(q0 + i) * a.q_stride + (size_t)ts * a.step_stride] = h;
          }
        }
        __syncthreads();
      }
    }
  }
  if constexpr (ROWS) {
    if (cell)
      for (int s = steps; s < a.steps; ++s) hrow[(size_t)(q0 + i) * a.q_stride + (size_t)s * a.step_stride] = 0.f;
  }
  if (cell) {
    const size_t off = ((size_t)n * DH + d * H + j) * a.ldq + q0 + i;
    if (a.h_last) a.h_last[off] = h;
    if (a.c_last) a.c_last[off] = c;
  }
}

// ---- GRU / Elman RNN cells (SingleRNN(rnn_type="GRU" | "RNN"), lobe/rnn.py:19-35: no recipe builds them) -------------------
// The structure of lstm_kernel<false>: LS sequences per workgroup, a thread per gate row that walks W_hh^T's column with h in
// LDS, then a thread per (unit, sequence) for the cell.  gx holds W_ih x + b_ih (+ b_hh except for the GRU's n gate, whose
// hidden bias sits inside the reset product: bhn [D][H]).  KIND 0: h' = tanh(gx + W_hh h); 2: GRU, gates r, z, n.
template <int KIND>
__global__ __launch_bounds__(1024) void rnn_kernel(LstmK k, const float* __restrict__ bhn) {
  constexpr int NG = KIND == 2 ? 3 : 1;
  extern __shared__ float smem[];
  const ps_lstm_args& a = k.a;
  const int H = a.H, G = NG * H;
  f32x4* hbuf = reinterpret_cast<f32x4*>(smem);  // [H]  current h of the LS sequences
  f32x4* abuf = hbuf + H;                          // [G]  W_hh h (+ gx, + b_hn)
  f32x4* xbuf = abuf + G;                          // [H]  GRU: gx of the n gate
  const int g = threadIdx.x;
  const int q0 = blockIdx.x * LS, n = blockIdx.y, d = blockIdx.z;
  const bool row = g < G;
  const int DH = a.D * H;
  const float* wt = a.whh_t + (size_t)d * H * G + g;
  const int j = g % H, i = g / H;  // cell role: unit j of sequence i
  const bool cell = g < H * LS && q0 + i < a.Q;
  float h = 0.f;
  if (cell && a.h0) h = a.h0[((size_t)n * DH + d * H + j) * a.ldq + q0 + i];
  if (g < H * LS) reinterpret_cast<float*>(hbuf)[j * LS + i] = h;
  const float* grow = a.gx + ((size_t)n * a.D * G + (size_t)d * G + g) * a.ldt;
  float* hrow = a.hout + ((size_t)n * DH + d * H + j) * a.ldt;
  const bool rev = d == 1;
  const float bn = (KIND == 2 && row && g >= 2 * H && bhn) ? bhn[d * H + (g - 2 * H)] : 0.f;
  __syncthreads();
  for (int s = 0; s < a.steps; ++s) {
    const int ts = rev ? a.steps - 1 - s : s;
    if (row) {
      f32x4 pre, acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < LS; ++e)
        pre[e] = q0 + e < a.Q ? grow[(size_t)(q0 + e) * a.q_stride + (size_t)ts * a.step_stride] : 0.f;
#pragma unroll 8
      for (int kk = 0; kk < H; ++kk) acc += wt[(size_t)kk * G] * hbuf[kk];
      if (KIND == 2 && g >= 2 * H) {
        abuf[g] = acc + bn;
        xbuf[g - 2 * H] = pre;
      } else {
        abuf[g] = acc + pre;
      }
    }
    __syncthreads();
    if (g < H * LS) {
      const float* ab = reinterpret_cast<const float*>(abuf);
      if constexpr (KIND == 2) {
        const float r = sigmoidf_(ab[j * LS + i]);
        const float z = sigmoidf_(ab[(H + j) * LS + i]);
        const float nn = tanhf(reinterpret_cast<const float*>(xbuf)[j * LS + i] + r * ab[(2 * H + j) * LS + i]);
        h = (1.f - z) * nn + z * h;
      } else {
        h = tanhf(ab[j * LS + i]);
      }
      reinterpret_cast<float*>(hbuf)[j * LS + i] = h;
      if (cell) hrow[(size_t)(q0 + i) * a.q_stride + (size_t)ts * a.step_stride] = h;
    }
    __syncthreads();
  }
  if (cell && a.h_last) a.h_last[((size_t)n * DH + d * H + j) * a.ldq + q0 + i] = h;
}

// ---- MFMA recurrence for H = 64 / 128 ----------------------------------------------------------------------------
// One workgroup owns 16 sequences (flat index b = n*Q + q, so a group may span two utterances) and H/16 waves; wave
// w owns hidden units [16w, 16w+16) and ALL FOUR gates of them, so the cell update needs no exchange:
//   D_g[unit][seq] = gx_g + W_hh,g[16 units x H] * h[H x 16 seqs]      g = i, f, g, o
// as 4 x H/4 v_mfma_f32_16x16x4_f32 per step with W_hh resident in VGPRs as A fragments.  C/D layout: lane (seq =
// lane&15, quad = lane>>4) holds units 4*quad + r of its wave in register r -- the same (unit, seq) position in all four
// gate accumulators -- so c, h stay in registers.  h' goes through LDS once per step ([k-block][quad][seq], written
// and read conflict-free) to become everybody's B fragments; the k axis is walked in the order (wave, r, quad) the
// producers hold it in, with W_hh's fragments loaded in the same order.
template <int H>
struct LstmMfma {
  static constexpr int NW = H / 16;  // waves
  static constexpr int KB = H / 4;   // k-blocks of 4
  static constexpr int PF = H == 64 ? 4 : 2;
};

__device__ __forceinline__ float fast_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
__device__ __forceinline__ float fast_tanh(float x) {
  return 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-2.88539008177792681f * x)) - 1.f;
}

template <int H, bool CONTIG>
__global__ __launch_bounds__(H * 4) void lstm_mfma_kernel(LstmK k) {
  using P = LstmMfma<H>;
  constexpr int KB = P::KB, PF = CONTIG ? 4 : P::PF;
  __shared__ float hbuf[2][H * 16];
  const ps_lstm_args& a = k.a;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int d = blockIdx.z;
  const int b = blockIdx.x * 16 + col;
  const bool valid = b < a.N * a.Q;
  const int n = valid ? b / a.Q : 0, q = valid ? b % a.Q : 0;
  const int G = 4 * H;
  const int unit0 = 16 * w + 4 * quad;  // first of this lane's 4 units

  // A fragments: gate g, k-block kb = (w', r'): A[row = lane&15][k = 16w' + 4*quad + r']
  float wf[4][KB];
  {
    const float* wt = a.whh_t + (size_t)d * H * G;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int kk = 16 * (kb >> 2) + 4 * quad + (kb & 3);
        wf[g][kb] = wt[(size_t)kk * G + g * H + 16 * w + col];
      }
  }

  float c[4] = {0.f, 0.f, 0.f, 0.f}, h[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid && (a.h0 || a.c0)) {
    const int bs = b - a.state_shift;
    if (bs >= 0) {
      const int nn = bs / a.Q, qq = bs % a.Q;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t off = ((size_t)(nn * a.D + d) * H + unit0 + r) * a.ldq + qq;
        if (a.h0) h[r] = a.h0[off];
        if (a.c0) c[r] = a.c0[off];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) hbuf[0][((w * 4 + r) * 4 + quad) * 16 + col] = h[r];

  const float* gp = a.gx + ((size_t)(n * a.D + d) * G + unit0) * a.ldt + (size_t)q * a.q_stride;
  float* hp = a.hout + ((size_t)(n * a.D + d) * H + unit0) * a.ldt + (size_t)q * a.q_stride;
  const int steps = a.steps;
  const bool rev = d == 1;
  const size_t ldt = a.ldt;

  // pre[u][g][r]: gate pre-activations of the step in ring slot u.  CONTIG (steps are consecutive frames, 16-byte
  // aligned groups of 4): one 16-byte load per (gate, unit) fetches a whole group of 4 steps, the next group is in
  // flight while this one is consumed, and h' leaves as 16-byte stores; otherwise scalar loads PF steps ahead.
  float pre[PF][4][4];
  f32x4 nxt[4][4];
  auto load_group = [&](int s0) {  // CONTIG: steps s0 .. s0+3 -> nxt
    const int f0 = rev ? steps - 4 - s0 : s0;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        nxt[g][r] = (valid && s0 < steps) ? *reinterpret_cast<const f32x4*>(gp + (size_t)(g * H + r) * ldt + f0)
                                          : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto take_group = [&]() {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) pre[u][g][r] = rev ? nxt[g][r][3 - u] : nxt[g][r][u];
  };
  if constexpr (CONTIG) {
    load_group(0);
  } else {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int ts = rev ? steps - 1 - u : u;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pre[u][g][r] = (valid && u < steps) ? gp[(size_t)(g * H + r) * ldt + (size_t)ts * a.step_stride] : 0.f;
    }
  }
  __syncthreads();

  for (int s0 = 0; s0 < steps; s0 += PF) {
    // CONTIG: h' of the group, [r][u].  A forward pass may end in a partial group, whose 16-byte store reaches up to 3 frames
    // past the last step: those are pad frames, and they get zeros (the rows of _plans._h_rows keep their pads zero)
    float hst[4][4] = {};
    if constexpr (CONTIG) {
      take_group();
      load_group(s0 + 4);
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int s = s0 + u;
      if (s < steps) {  // uniform
        const float* hb = hbuf[s & 1];
        float bf[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) bf[kb] = hb[kb * 64 + lane];
        f32x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = f32x4{pre[u][g][0], pre[u][g][1], pre[u][g][2], pre[u][g][3]};
        if constexpr (!CONTIG) {  // refill the ring slot with step s + PF
          const int sn = s + PF;
          const int ts = rev ? steps - 1 - sn : sn;
          if (sn < steps) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                pre[u][g][r] = valid ? gp[(size_t)(g * H + r) * ldt + (size_t)ts * a.step_stride] : 0.f;
          }
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[g][kb], bf[kb], acc[g], 0, 0, 0);
        float* hn = hbuf[(s + 1) & 1];
        const int ts = rev ? steps - 1 - s : s;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gi = fast_sigmoid(acc[0][r]);
          const float gf = fast_sigmoid(acc[1][r]);
          const float gg = fast_tanh(acc[2][r]);
          const float go = fast_sigmoid(acc[3][r]);
          c[r] = gf * c[r] + gi * gg;
          h[r] = go * fast_tanh(c[r]);
          hn[((w * 4 + r) * 4 + quad) * 16 + col] = h[r];
          if constexpr (CONTIG) {
            hst[r][rev ? 3 - u : u] = h[r];
          } else {
            if (valid) hp[(size_t)r * ldt + (size_t)ts * a.step_stride] = h[r];
          }
        }
        __syncthreads();
      }
    }
    if constexpr (CONTIG) {
      if (valid) {
        const int f0 = rev ? steps - 4 - s0 : s0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<f32x4*>(hp + (size_t)r * ldt + f0) = f32x4{hst[r][0], hst[r][1], hst[r][2], hst[r][3]};
      }
    }
  }
  if (valid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t off = ((size_t)(n * a.D + d) * H + unit0 + r) * a.ldq + q;
      if (a.h_last) a.h_last[off] = h[r];
      if (a.c_last) a.c_last[off] = c[r];
    }
  }
}

// ---- whole-segment MFMA recurrence (intra-segment pass: many short sequences of consecutive frames) ---------------
// The 16-sequence kernel above fetches the gate pre-activations in 16-byte groups of 4 steps, one group ahead: with
// q_stride = K frames (K = 20: 80 bytes) each 128-byte line of a gate row holds 1.6 whole sequences and is visited
// by all five groups, ~6 us apart; 64 resident workgroups per XCD keep 21 MB of such lines in flight against a 4 MB
// L2, so every visit misses: 645 MB fetched for 131 MB of pre-activations (profiles/r03_pmc_cfg4_traffic_group_kernel.txt) and the
// pass runs at the fabric's rate, not the recurrence's.  Here a workgroup fetches ALL the steps of its 16 sequences
// before the first one (the five groups of a line leave back to back and merge in the vector L1 / L2), keeps them
// in registers -- STEPS x 16 values per lane, the reason for one wave per SIMD (__launch_bounds__(256, 1): 512
// registers) -- and stages h' in LDS so that it leaves as whole 16-sequence x STEPS-frame rows of 16-byte stores.
template <int H, int STEPS, bool BIDIR>
__global__ __launch_bounds__(H * 4, 1) void lstm_seg_kernel(LstmK k) {
  static_assert(H == 64 && STEPS % 4 == 0, "16 units per wave, 4 waves; steps in 16-byte groups");
  constexpr int KB = H / 4, NG = STEPS / 4;
  constexpr int LDH = 16 * STEPS + 4;  // staged h' row: [unit][seq * STEPS + frame], 16-byte aligned rows
  __shared__ __attribute__((aligned(16))) float hbuf[2][H * 16];
  __shared__ __attribute__((aligned(16))) float hstage[H * LDH];
  __shared__ long long seq_off[16];
  const ps_lstm_args& a = k.a;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int d = blockIdx.z;
  const int b = blockIdx.x * 16 + col;
  const bool valid = b < a.N * a.Q;
  // sequences past the end (the last workgroup) replay the last real one: every load below is unconditional -- a guarded
  // load is an exec-mask branch each, and one of them made the compiler wait for ALL outstanding loads -- and nothing of
  // theirs is stored (seq_off < 0, `valid` around the final states)
  const int bb = valid ? b : a.N * a.Q - 1;
  const int n = bb / a.Q, q = bb % a.Q;
  const int G = 4 * H;
  const int unit0 = 16 * w + 4 * quad;
  const bool rev = BIDIR && d == 1;  // (one direction: the loads land in their final registers, no selects)
  const size_t ldt = a.ldt;

  if (threadIdx.x < 16) seq_off[threadIdx.x] = valid ? (long long)((size_t)(n * a.D + d) * H * ldt + (size_t)q * a.q_stride) : -1;

  // recurrent weights and initial states first: loads return in order, and these are needed before step 0
  float wf[4][KB];
  {
    const float* wt = a.whh_t + (size_t)d * H * G;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int kk = 16 * (kb >> 2) + 4 * quad + (kb & 3);
        wf[g][kb] = wt[(size_t)kk * G + g * H + 16 * w + col];
      }
  }

  float c[4] = {0.f, 0.f, 0.f, 0.f}, h[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid && (a.h0 || a.c0)) {
    const int bs = b - a.state_shift;
    if (bs >= 0) {
      const int nn = bs / a.Q, qq = bs % a.Q;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t off = ((size_t)(nn * a.D + d) * H + unit0 + r) * a.ldq + qq;
        if (a.h0) h[r] = a.h0[off];
        if (a.c0) c[r] = a.c0[off];
      }
    }
  }

  // every step's pre-activations: pre[s][g][r], s in processing order (frame STEPS-1-s for the reverse direction)
  float pre[STEPS][4][4];
  {
    const float* gp = a.gx + ((size_t)(n * a.D + d) * G + unit0) * ldt + (size_t)q * a.q_stride;
    // (the five 16-byte groups of a row back to back: they share a 128-byte line and merge on the way to the L2; with the
    //  step groups outermost -- first steps startable earlier -- the kernel took 72 us instead of 61)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < NG; ++j) {
          const int jj = rev ? NG - 1 - j : j;
          const f32x4 v = *reinterpret_cast<const f32x4*>(gp + (size_t)(g * H + r) * ldt + 4 * jj);
#pragma unroll
          for (int e = 0; e < 4; ++e) pre[4 * j + e][g][r] = rev ? v[3 - e] : v[e];
        }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) hbuf[0][((w * 4 + r) * 4 + quad) * 16 + col] = h[r];
  __syncthreads();

#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const float* hb = hbuf[s & 1];
    float bf[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) bf[kb] = hb[kb * 64 + lane];
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{pre[s][g][0], pre[s][g][1], pre[s][g][2], pre[s][g][3]};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[g][kb], bf[kb], acc[g], 0, 0, 0);
    float* hn = hbuf[(s + 1) & 1];
    const int f = rev ? STEPS - 1 - s : s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = fast_sigmoid(acc[0][r]);
      const float gf = fast_sigmoid(acc[1][r]);
      const float gg = fast_tanh(acc[2][r]);
      const float go = fast_sigmoid(acc[3][r]);
      c[r] = gf * c[r] + gi * gg;
      h[r] = go * fast_tanh(c[r]);
      hn[((w * 4 + r) * 4 + quad) * 16 + col] = h[r];
      hstage[(unit0 + r) * LDH + col * STEPS + f] = h[r];
    }
    __syncthreads();
  }

  // h' rows: 16 sequences x STEPS frames per unit, 16 bytes per store (the last barrier of the loop covers hstage)
  for (int p = threadIdx.x; p < H * 16 * NG; p += H * 4) {
    const int unit = p / (16 * NG), rem = p % (16 * NG);
    const int sq = rem / NG, gr = rem % NG;
    const long long off = seq_off[sq];
    if (off >= 0)
      *reinterpret_cast<f32x4*>(a.hout + off + (size_t)unit * ldt + 4 * gr) =
          *reinterpret_cast<const f32x4*>(&hstage[unit * LDH + sq * STEPS + 4 * gr]);
  }
  if (valid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t off = ((size_t)(n * a.D + d) * H + unit0 + r) * a.ldq + q;
      if (a.h_last) a.h_last[off] = h[r];
      if (a.c_last) a.c_last[off] = c[r];
    }
  }
}

// ---- the same with the recurrent product W_hh h in two fp16 terms per operand (ps_lstm_f16x2_f32) -----------------
// 64 v_mfma_f32_16x16x4_f32 per step (2048 cycles of the matrix pipe, two thirds of the step) become 24
// v_mfma_f32_16x16x32_f16 (384 cycles): W_hh * 2^e = W_hi + W_lo once per workgroup (e puts the largest |weight| into
// [2^12, 2^13)), h * 2^10 = h_hi + h_lo every step (|h| < 1), three products hi*hi + hi*lo + lo*hi accumulated in
// fp32 on top of the (scaled) fp32 pre-activations; the scale comes out again, exactly, before the cell non-linearities.
// Dropped: the lo*lo term and the fp16 rounding of the two lo parts, together <= 2^-21 of sum_k |W_k| |h_k| per gate -- the
// class of the fp16x2 GEMM that produced the pre-activations.  C/D layout as the 16x16x4 instruction, so the cell and
// the staging are the fp32 kernel's; h' crosses LDS as [plane][sequence][k] halves (8-byte writes, 16-byte reads).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

template <int H, int STEPS, bool BIDIR>
__global__ __launch_bounds__(H * 4, 1) void lstm_seg_f16x2_kernel(LstmK k) {
  static_assert(H == 64 && STEPS % 4 == 0, "16 units per wave, 4 waves; steps in 16-byte groups");
  constexpr int NG = STEPS / 4;
  constexpr int LDH = 16 * STEPS + 4;
  constexpr int LDK = H + 8;  // halves per (plane, sequence) row: 144 bytes, conflict-free 8-byte writes / 16-byte reads
  __shared__ __attribute__((aligned(16))) _Float16 hb[2][2][16][LDK];
  __shared__ __attribute__((aligned(16))) float hstage[H * LDH];
  __shared__ long long seq_off[16];
  __shared__ float wmax[4];
  const ps_lstm_args& a = k.a;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int d = blockIdx.z;
  const int b = blockIdx.x * 16 + col;
  const bool valid = b < a.N * a.Q;
  // sequences past the end (the last workgroup) replay the last real one: every load below is unconditional -- a guarded
  // load is an exec-mask branch each, and one of them made the compiler wait for ALL outstanding loads -- and nothing of
  // theirs is stored (seq_off < 0, `valid` around the final states)
  const int bb = valid ? b : a.N * a.Q - 1;
  const int n = bb / a.Q, q = bb % a.Q;
  const int G = 4 * H;
  const int unit0 = 16 * w + 4 * quad;
  const bool rev = BIDIR && d == 1;  // (one direction: the loads land in their final registers, no selects)
  const size_t ldt = a.ldt;

  if (threadIdx.x < 16) seq_off[threadIdx.x] = valid ? (long long)((size_t)(n * a.D + d) * H * ldt + (size_t)q * a.q_stride) : -1;

  // A fragments: gate g, k-step ks: lane (row = lane & 15 -> unit 16 w + row, k-group = lane >> 4) holds k = 32 ks + 8 kgroup + e
  // Issue order: the 64 recurrent weights of this lane, then all STEPS x 16 pre-activations, THEN the weights' maximum,
  // scale and split -- the weights return first (loads return in order) and are processed under the pre-activations'
  // flight instead of in front of it.
  const float* wt = a.whh_t + (size_t)d * H * G;
  float wv[4][2][8];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) wv[g][ks][e] = wt[(size_t)(32 * ks + 8 * quad + e) * G + g * H + 16 * w + col];

  // (initial states next: loads return in order, and these are waited for before step 0)
  float c[4] = {0.f, 0.f, 0.f, 0.f}, h[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid && (a.h0 || a.c0)) {
    const int bs = b - a.state_shift;
    if (bs >= 0) {
      const int nn = bs / a.Q, qq = bs % a.Q;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t off = ((size_t)(nn * a.D + d) * H + unit0 + r) * a.ldq + qq;
        if (a.h0) h[r] = a.h0[off];
        if (a.c0) c[r] = a.c0[off];
      }
    }
  }

  float pre[STEPS][4][4];
  {
    const float* gp = a.gx + ((size_t)(n * a.D + d) * G + unit0) * ldt + (size_t)q * a.q_stride;
    // (the five 16-byte groups of a row back to back: they share a 128-byte line and merge on the way to the L2; with the
    //  step groups outermost -- first steps startable earlier -- the kernel took 72 us instead of 61)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < NG; ++j) {
          const int jj = rev ? NG - 1 - j : j;
          const f32x4 v = *reinterpret_cast<const f32x4*>(gp + (size_t)(g * H + r) * ldt + 4 * jj);
#pragma unroll
          for (int e = 0; e < 4; ++e) pre[4 * j + e][g][r] = rev ? v[3 - e] : v[e];
        }
  }


  f16x8 whi[4][2], wlo[4][2];
  float inv;
  {
    float m = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(wv[g][ks][e]));
    m = wave_max(m);
    if (lane == 0) wmax[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    int ex = 0;
    if (m > 0.f) frexpf(m, &ex);  // m = f * 2^ex, f in [0.5, 1)
    ex = ex < -27 ? -27 : ex;     // (tiny matrices: keep the scaled products far from overflow)
    const float S = ldexpf(1.f, 13 - ex);
    inv = 1.f / (S * 1024.f);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float ws = wv[g][ks][e] * S;
          const _Float16 hi = (_Float16)ws;
          whi[g][ks][e] = hi;
          wlo[g][ks][e] = (_Float16)(ws - (float)hi);
        }
  }

  auto put_h = [&](int buf) {  // this lane's 4 units of sequence `col`: two 8-byte writes
    f16x4 hi4, lo4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float hs = h[r] * 1024.f;
      const _Float16 hi = (_Float16)hs;
      hi4[r] = hi;
      lo4[r] = (_Float16)(hs - (float)hi);
    }
    *reinterpret_cast<f16x4*>(&hb[buf][0][col][unit0]) = hi4;
    *reinterpret_cast<f16x4*>(&hb[buf][1][col][unit0]) = lo4;
  };
  put_h(0);
  __syncthreads();

#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    f16x8 bh[2][2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) bh[pl][ks] = *reinterpret_cast<const f16x8*>(&hb[s & 1][pl][col][32 * ks + 8 * quad]);
    f32x4 acc[4];  // starts at zero: the fp32 pre-activation joins after the scale has come out (one fma per value)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[g][ks], bh[0][ks], acc[g], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[g][ks], bh[1][ks], acc[g], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wlo[g][ks], bh[0][ks], acc[g], 0, 0, 0);
    const int f = rev ? STEPS - 1 - s : s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = fast_sigmoid(fmaf(acc[0][r], inv, pre[s][0][r]));
      const float gf = fast_sigmoid(fmaf(acc[1][r], inv, pre[s][1][r]));
      const float gg = fast_tanh(fmaf(acc[2][r], inv, pre[s][2][r]));
      const float go = fast_sigmoid(fmaf(acc[3][r], inv, pre[s][3][r]));
      c[r] = gf * c[r] + gi * gg;
      h[r] = go * fast_tanh(c[r]);
      hstage[(unit0 + r) * LDH + col * STEPS + f] = h[r];
    }
    put_h((s + 1) & 1);
    __syncthreads();
  }

  for (int p = threadIdx.x; p < H * 16 * NG; p += H * 4) {
    const int unit = p / (16 * NG), rem = p % (16 * NG);
    const int sq = rem / NG, gr = rem % NG;
    const long long off = seq_off[sq];
    if (off >= 0)
      *reinterpret_cast<f32x4*>(a.hout + off + (size_t)unit * ldt + 4 * gr) =
          *reinterpret_cast<const f32x4*>(&hstage[unit * LDH + sq * STEPS + 4 * gr]);
  }
  if (valid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t off = ((size_t)(n * a.D + d) * H + unit0 + r) * a.ldq + q;
      if (a.h_last) a.h_last[off] = h[r];
      if (a.c_last) a.c_last[off] = c[r];
    }
  }
}

// ---- 4-sequence MFMA recurrence (v_mfma_f32_4x4x1_16B_f32) -------------------------------------------------------
// For passes with few, long sequences (the inter-segment pass: N*K sequences of S steps) the 16-sequence kernel above
// leaves most CUs idle and walks the steps at ~2 us each.  Here a workgroup owns only 4 sequences.  The instruction
// multiplies 16 independent 4x4 blocks: block = hidden unit (16 per wave), block row = gate (i, f, g, o), block column
// = sequence, K = 1 per issue, so lane (unit b, sequence j) receives the four gate pre-activations of ITS (unit,
// sequence) in the four result registers and does the cell update alone.  A = W_hh[gate][unit][k] resident (H VGPRs),
// B = h[k][sequence] broadcast from LDS.  Four independent accumulators hide the dependent-issue latency.
template <int H, bool CONTIG>
__global__ __launch_bounds__(H * 4) void lstm_m4_kernel(LstmK k) {
  constexpr int HS = H + 16;  // LDS row stride: conflict-free h' writes
  constexpr int PF = CONTIG ? 4 : 8;
  __shared__ __attribute__((aligned(16))) float hbuf[2][4 * HS];
  const ps_lstm_args& a = k.a;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = lane & 3, ub = lane >> 2;
  const int unit = 16 * w + ub;
  const int d = blockIdx.z;
  // XCD-aware group order: consecutive workgroup ids are dealt round-robin to the 8 XCDs (each with its own L2), but
  // neighbouring sequence groups share the 128-byte lines of the gate rows (4 sequences = 16 bytes of a line), so
  // groups are renumbered to put neighbours on ONE XCD: id -> (id % 8) * ceil(G/8) + id / 8.
  // (the grid is a multiple of 8 groups, so this is a bijection; groups past the last sequence are masked by `valid`)
  const int per = gridDim.x >> 3;
  const int grp = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const int b = grp * 4 + j;
  const bool valid = b < a.N * a.Q;
  // sequences past the end replay the last real one: the gate loads of the step loop are unconditional (a guarded load is
  // an exec-mask branch in the dependent chain of every step); nothing of theirs is stored
  const int bb = valid ? b : a.N * a.Q - 1;
  const int n = bb / a.Q, q = bb % a.Q;
  const int G = 4 * H;

  // A operand: lane (unit, i = lane&3) holds W_hh[gate i][unit][k]
  float wf[H];
  {
    const float* wt = a.whh_t + (size_t)d * H * G + j * H + unit;
#pragma unroll
    for (int kk = 0; kk < H; ++kk) wf[kk] = wt[(size_t)kk * G];
  }

  float c = 0.f, h = 0.f;
  if (valid && (a.h0 || a.c0)) {
    const int bs = b - a.state_shift;
    if (bs >= 0) {
      const int nn = bs / a.Q, qq = bs % a.Q;
      const size_t off = ((size_t)(nn * a.D + d) * H + unit) * a.ldq + qq;
      if (a.h0) h = a.h0[off];
      if (a.c0) c = a.c0[off];
    }
  }
  hbuf[0][j * HS + unit] = h;

  const float* gp = a.gx + ((size_t)(n * a.D + d) * G + unit) * a.ldt + (size_t)q * a.q_stride;
  float* hp = a.hout + ((size_t)(n * a.D + d) * H + unit) * a.ldt + (size_t)q * a.q_stride;
  const int steps = a.steps;
  const bool rev = d == 1;
  const size_t gstride = (size_t)H * a.ldt;  // between the gates of one unit

  float pre[PF][4];
  f32x4 nxt[4];
  auto load_group = [&](int s0) {  // CONTIG: steps s0 .. s0+3 of every gate -> nxt
    const int f0 = rev ? steps - 4 - s0 : s0;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      nxt[g] = (valid && s0 < steps) ? *reinterpret_cast<const f32x4*>(gp + g * gstride + f0)
                                     : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  if constexpr (CONTIG) {
    load_group(0);
  } else {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int uc = u < steps ? u : steps - 1;
      const int ts = rev ? steps - 1 - uc : uc;
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[u][g] = gp[g * gstride + (size_t)ts * a.step_stride];
    }
  }
  __syncthreads();

  for (int s0 = 0; s0 < steps; s0 += PF) {
    float hst[4] = {};  // (a partial last group stores zeros into the pad frames past the last step, as lstm_mfma_kernel)
    if constexpr (CONTIG) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[u][g] = rev ? nxt[g][3 - u] : nxt[g][u];
      load_group(s0 + 4);
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int s = s0 + u;
      if (s < steps) {  // uniform
        const float* hb = hbuf[s & 1] + j * HS;
        f32x4 acc[2];
        acc[0] = f32x4{pre[u][0], pre[u][1], pre[u][2], pre[u][3]};
        acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#ifndef PS_M4_ABL
#define PS_M4_ABL 0
#endif
#pragma unroll
        for (int kk = 0; kk < ((PS_M4_ABL & 1) ? 1 : H / 4); ++kk) {
          const f32x4 hv = *reinterpret_cast<const f32x4*>(hb + 4 * kk);
#pragma unroll
          for (int e = 0; e < 4; ++e)  // two accumulator chains (116 us per inter pass; four: 119, one: 130)
            acc[e & 1] = __builtin_amdgcn_mfma_f32_4x4x1f32(wf[4 * kk + e], hv[e], acc[e & 1], 0, 0, 0);
        }
        if constexpr (!CONTIG) {
          // refill the ring slot with step s + PF -- behind the MFMAs (in front of them the four loads and their
          // address arithmetic sat between the barrier and the first LDS read of the step's dependent chain); steps past
          // the end re-read the last one
          const int sn = s + PF < steps ? s + PF : steps - 1;
          const int ts = rev ? steps - 1 - sn : sn;
#pragma unroll
          for (int g = 0; g < 4; ++g) pre[u][g] = gp[g * gstride + (size_t)ts * a.step_stride];
          // ... and the PREVIOUS step's h' leaves here too (same reason; the last one after the loop)
          if (s > 0 && valid) hp[(size_t)(rev ? steps - s : s - 1) * a.step_stride] = h;
        }
        const f32x4 t = acc[0] + acc[1];
#if PS_M4_ABL & 2
        c = t[1] * c + t[0] * t[2];
        h = t[3] * c;
#else
        const float gi = fast_sigmoid(t[0]);
        const float gf = fast_sigmoid(t[1]);
        const float gg = fast_tanh(t[2]);
        const float go = fast_sigmoid(t[3]);
        c = gf * c + gi * gg;
        h = go * fast_tanh(c);
#endif
        hbuf[(s + 1) & 1][j * HS + unit] = h;
        __syncthreads();
        if constexpr (CONTIG) {
          hst[rev ? 3 - u : u] = h;
        }
      }
    }
    if constexpr (CONTIG) {
      if (valid) {
        const int f0 = rev ? steps - 4 - s0 : s0;
        *reinterpret_cast<f32x4*>(hp + f0) = f32x4{hst[0], hst[1], hst[2], hst[3]};
      }
    }
  }
  if constexpr (!CONTIG) {
    if (valid) hp[(size_t)(rev ? 0 : steps - 1) * a.step_stride] = h;
  }
  if (valid) {
    const size_t off = ((size_t)(n * a.D + d) * H + unit) * a.ldq + q;
    if (a.h_last) a.h_last[off] = h;
    if (a.c_last) a.c_last[off] = c;
  }
}

// ---- the 4-sequence recurrence with the product W_hh h in two fp16 terms (ps_lstm_f16x2_f32, inter-segment pass) --------
// The step of lstm_m4_kernel is a dependent chain: 64 v_mfma_f32_4x4x1_f32 (512 cycles of issue), the cell, one LDS
// exchange.  v_mfma_f32_4x4x4_f16 takes four k per issue: with W_hh 2^e = hi + lo once per workgroup and h 2^10 = hi +
// lo every step (the scheme of lstm_seg_f16x2_kernel, same error class) the chain is 3 x 16 issues, 384 cycles.  Layout
// as the fp32 kernel: lane (unit, j): A = W_hh[gate j][unit][4 k], B = h[4 k][sequence j], the four result registers
// the four gates of (unit, sequence j).  h' crosses LDS as halves, [plane][sequence][k], read 16 bytes (8 k) at a time.
typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void lstm_m4_f16x2_kernel(LstmK k) {
  constexpr int H = 64, PF = 8;
  constexpr int LDK = H + 8;  // halves per (plane, sequence) row
  __shared__ __attribute__((aligned(16))) _Float16 hb[2][2][4][LDK];
  __shared__ float wmax[4];
  const ps_lstm_args& a = k.a;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = lane & 3, ub = lane >> 2;
  const int unit = 16 * w + ub;
  const int d = blockIdx.z;
  const int per = gridDim.x >> 3;  // XCD-aware group order, as lstm_m4_kernel
  const int grp = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const int b = grp * 4 + j;
  const bool valid = b < a.N * a.Q;
  const int bb = valid ? b : a.N * a.Q - 1;  // (sequences past the end replay the last one; nothing of theirs is stored)
  const int n = bb / a.Q, q = bb % a.Q;
  const int G = 4 * H;

  // A operand: lane (unit, i = lane & 3) holds W_hh[gate i][unit][k], k-step kk: k = 4 kk .. 4 kk + 3
  f16x4v whi[H / 4], wlo[H / 4];
  float inv;
  {
    const float* wt = a.whh_t + (size_t)d * H * G + j * H + unit;
    float wv[H];
    float m = 0.f;
#pragma unroll
    for (int kk = 0; kk < H; ++kk) {
      wv[kk] = wt[(size_t)kk * G];
      m = fmaxf(m, fabsf(wv[kk]));
    }
    m = wave_max(m);
    if (lane == 0) wmax[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    int ex = 0;
    if (m > 0.f) frexpf(m, &ex);
    ex = ex < -27 ? -27 : ex;
    const float S = ldexpf(1.f, 13 - ex);
    inv = 1.f / (S * 1024.f);
#pragma unroll
    for (int kk = 0; kk < H / 4; ++kk)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ws = wv[4 * kk + e] * S;
        const _Float16 hi = (_Float16)ws;
        whi[kk][e] = hi;
        wlo[kk][e] = (_Float16)(ws - (float)hi);
      }
  }

  float c = 0.f, h = 0.f;
  if (a.h0 || a.c0) {  // (replayed sequences take the replayed state: they must store the very same h')
    const int bs = bb - a.state_shift;
    if (bs >= 0) {
      const int nn = bs / a.Q, qq = bs % a.Q;
      const size_t off = ((size_t)(nn * a.D + d) * H + unit) * a.ldq + qq;
      if (a.h0) h = a.h0[off];
      if (a.c0) c = a.c0[off];
    }
  }
  auto put_h = [&](int buf) {
    const float hs = h * 1024.f;
    const _Float16 hi = (_Float16)hs;
    hb[buf][0][j][unit] = hi;
    hb[buf][1][j][unit] = (_Float16)(hs - (float)hi);
  };
  put_h(0);

  const float* gp = a.gx + ((size_t)(n * a.D + d) * G + unit) * a.ldt + (size_t)q * a.q_stride;
  float* hp = a.hout + ((size_t)(n * a.D + d) * H + unit) * a.ldt + (size_t)q * a.q_stride;
  const int steps = a.steps;
  const bool rev = d == 1;
  const size_t gstride = (size_t)H * a.ldt;

  float pre[PF][4];
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const int uc = u < steps ? u : steps - 1;
    const int ts = rev ? steps - 1 - uc : uc;
#pragma unroll
    for (int g = 0; g < 4; ++g) pre[u][g] = gp[g * gstride + (size_t)ts * a.step_stride];
  }
  __syncthreads();

  for (int s0 = 0; s0 < steps; s0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int s = s0 + u;
      if (s < steps) {  // uniform
        const _Float16* hh = &hb[s & 1][0][j][0];
        const _Float16* hl = &hb[s & 1][1][j][0];
        constexpr int NC = 2;  // accumulator chains: 105 us with two, 108 with four, 110 with one, 115 with six
        f32x4 acc[NC];
#pragma unroll
        for (int e = 0; e < NC; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 p4 = f32x4{pre[u][0], pre[u][1], pre[u][2], pre[u][3]};
#pragma unroll
        for (int k8 = 0; k8 < H / 8; ++k8) {
          const f16x8 vh = *reinterpret_cast<const f16x8*>(hh + 8 * k8);
          const f16x8 vl = *reinterpret_cast<const f16x8*>(hl + 8 * k8);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int kk = 2 * k8 + e;
            const f16x4v bh = f16x4v{vh[4 * e], vh[4 * e + 1], vh[4 * e + 2], vh[4 * e + 3]};
            const f16x4v bl = f16x4v{vl[4 * e], vl[4 * e + 1], vl[4 * e + 2], vl[4 * e + 3]};
            const int c0 = (3 * kk) % NC, c1 = (3 * kk + 1) % NC, c2 = (3 * kk + 2) % NC;
            acc[c0] = __builtin_amdgcn_mfma_f32_4x4x4f16(whi[kk], bh, acc[c0], 0, 0, 0);
            acc[c1] = __builtin_amdgcn_mfma_f32_4x4x4f16(whi[kk], bl, acc[c1], 0, 0, 0);
            acc[c2] = __builtin_amdgcn_mfma_f32_4x4x4f16(wlo[kk], bh, acc[c2], 0, 0, 0);
          }
        }
        {  // refill the ring slot (step s + PF) and let the previous step's h' leave: in the shadow of the MFMAs
          const int sn = s + PF < steps ? s + PF : steps - 1;
          const int ts = rev ? steps - 1 - sn : sn;
#pragma unroll
          for (int g = 0; g < 4; ++g) pre[u][g] = gp[g * gstride + (size_t)ts * a.step_stride];
          // (guarded: made unconditional -- replayed sequences storing the same values -- the kernel took 134 us, not 107)
          if (s > 0 && valid) hp[(size_t)(rev ? steps - s : s - 1) * a.step_stride] = h;
        }
        f32x4 sum = acc[0];
#pragma unroll
        for (int e = 1; e < NC; ++e) sum += acc[e];
        const f32x4 t = sum * inv + p4;
        const float gi = fast_sigmoid(t[0]);
        const float gf = fast_sigmoid(t[1]);
        const float gg = fast_tanh(t[2]);
        const float go = fast_sigmoid(t[3]);
        c = gf * c + gi * gg;
        h = go * fast_tanh(c);
        put_h((s + 1) & 1);
        __syncthreads();
      }
    }
  }
  if (valid) {
    hp[(size_t)(rev ? 0 : steps - 1) * a.step_stride] = h;
    const size_t off = ((size_t)(n * a.D + d) * H + unit) * a.ldq + q;
    if (a.h_last) a.h_last[off] = h;
    if (a.c_last) a.c_last[off] = c;
  }
}

typedef unsigned u32x4l __attribute__((ext_vector_type(4)));
#include "lstm_fm.inc"
typedef float f32x2 __attribute__((ext_vector_type(2)));
#include "lstm_fm256.inc"
#include "lstm_coop.inc"
#include "lstm_fm256_f32.inc"

}  // namespace ps

// the cooperative kernel's counters (a kernel, not hipMemsetAsync: inside a replayed graph a memset node does not have to go
// through the L2 the counters' atomics work in -- the first graph replays of that launch computed with the previous replay's counts)
__global__ __launch_bounds__(256) void zero_words_kernel(unsigned* p, int n) {
  for (int i = threadIdx.x; i < n; i += 256) p[i] = 0u;
}

using namespace ps;

// ---- checks: predicates on ps_lstm_args; every entry composes them and keeps its own message and return code ------------
// non-null gx / hout (and whh_t where the kernel reads it), D = 1 or 2, positive sizes, non-negative strides
static bool sizes_ok(const ps_lstm_args& a, bool reads_whh_t = true) {
  return a.gx && a.hout && (a.whh_t || !reads_whh_t) && a.N > 0 && a.H > 0 && a.D >= 1 && a.D <= 2 && a.Q > 0 && a.steps > 0 &&
         a.q_stride >= 0 && a.step_stride >= 0 && a.ldt > 0;
}
static long long last_frame(const ps_lstm_args& a) { return (long long)(a.Q - 1) * a.q_stride + (long long)(a.steps - 1) * a.step_stride; }
static bool has_states(const ps_lstm_args& a) { return a.h0 || a.c0 || a.h_last || a.c_last; }
// all state tensors of a launch are read and written with the row stride ldq
static bool states_ok(const ps_lstm_args& a) { return !has_states(a) || a.ldq >= a.Q; }
static bool shift_ok(const ps_lstm_args& a, int max_shift) { return a.state_shift >= 0 && a.state_shift <= max_shift; }
// frame-major gx [N][ldt][ldm]: 16-byte frames that hold the D*4H gate rows, 4-byte aligned hout
static bool fmajor_ok(const ps_lstm_args& a, int ldm) {
  return ldm >= a.D * 4 * a.H && ldm % 4 == 0 && !((uintptr_t)a.gx & 15) && !((uintptr_t)a.hout & 3);
}

// (no message: the probe of a caller choosing its path)
static bool lstm_fmajor_fits(const ps_lstm_args& a, int ldm) {
  return sizes_ok(a) && a.H == 128 && !has_states(a) && shift_ok(a, 0) && last_frame(a) < a.ldt && fmajor_ok(a, ldm) &&
         (long long)a.ldt * ldm * 4 < (1LL << 31) && (long long)a.ldt * 128 * 4 < (1LL << 31) &&
         (long long)a.N * ((a.Q + 15) / 16) < (1LL << 30);
}

static bool lstm_h256_fits(const ps_lstm_args& a, int ldm) {
  return sizes_ok(a, false) && (a.H == 256 || a.H == 192) && shift_ok(a, 1) && last_frame(a) < a.ldt && fmajor_ok(a, ldm) &&
         states_ok(a) && (long long)a.N * a.Q < (1LL << 30);
}

// channel-major gx, exact fp32 product (ps_lstm_h256_f32): the utterances that 16 consecutive flat sequences can touch lie
// under one buffer descriptor of the kernel, so their gx must stay below 2 GiB
static int h256_f32_span(const ps_lstm_args& a) {
  const long long span = (15 + (long long)a.Q - 1) / a.Q + 1;
  return (int)(span < a.N ? span : a.N);
}
static bool lstm_h256_f32_fits(const ps_lstm_args& a) {
  return sizes_ok(a, false) && (a.H == 256 || a.H == 192) && shift_ok(a, 1) && last_frame(a) < a.ldt && states_ok(a) &&
         !((uintptr_t)a.gx & 3) && !((uintptr_t)a.hout & 3) && (long long)a.N * a.Q < (1LL << 30) &&
         (long long)h256_f32_span(a) * a.D * 4 * a.H * a.ldt * 4 < (1LL << 31);
}

// ---- dispatch: store widths, the cooperative launch's layout, the kernel choice ------------------------------------------
// 8-byte h' stores of the h256 and cooperative kernels: consecutive frames in pairs that start on an 8-byte boundary
// (PS_DBG_LSTM_4B_STORES keeps the 4-byte ones: tests run both)
static bool store_pairs(const ps_lstm_args& a) {
  return a.step_stride == 1 && a.q_stride % 2 == 0 && a.ldt % 2 == 0 && !((uintptr_t)a.hout & 7) &&
         (a.D == 1 || a.steps % 2 == 0) && !dbg(PS_DBG_LSTM_4B_STORES);
}

// 16-byte step groups: steps are consecutive frames starting on a 16-byte boundary.  A forward-only pass may end
// in a partial group: it reads up to 3 frames past its last step and writes zeros there, which must still lie inside
// the row (pad frames; they are never read as data, but projection, LayerNorm and range maxima run over them).
// Without the groups a long pass over consecutive frames re-fetches every 128-byte line of the gate pre-activations
// once per step (DPCRN's inter pass: 10.8 ms instead of ~3).
// gx_too: gx is read in groups as well (channel-major gx; the frame-major entry has its gx rule in lstm_fmajor_fits).
static bool step_groups(const ps_lstm_args& a, bool gx_too) {
  const int steps4 = (a.steps + 3) / 4 * 4;
  const bool tail_ok = a.steps % 4 == 0 || (a.D == 1 && (long long)(a.Q - 1) * a.q_stride + steps4 <= a.ldt);
  return a.step_stride == 1 && tail_ok && a.q_stride % 4 == 0 && a.ldt % 4 == 0 && !(gx_too && ((uintptr_t)a.gx & 15)) &&
         !((uintptr_t)a.hout & 15);
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// The cooperative kernel: the streamed kernel's shapes, few enough sequence groups that every slice of every group gets a CU
// of its own at the same time (the group barrier spins: co-residency is a correctness condition, not a tuning choice).
// Workspace: the h exchange (hx_bytes), then sync_words counters, error word and XCD notes (hip._coop_layout mirrors it).
struct CoopLayout {
  int waves;           // per workgroup (= 16-unit row blocks per slice); 0: the launch does not fit
  bool per_direction;  // both directions do not fit at once: one launch per direction
  int groups;          // of 16 sequences
  size_t hx_bytes, sync_words, bytes;
};

// waves: 2 when the launch then still fits the chip -- more, smaller slices measured faster per step with a handful of
// groups (the speaker LSTM: 9.5 ms against 13.6) -- else 4, else 4 per direction if a direction fits, else 0
static CoopLayout coop_layout(const ps_lstm_args& a, int ldm) {
  CoopLayout l{};
  if (!lstm_h256_fits(a, ldm) || a.steps < 2) return l;
  const long long groups = ((long long)a.N * a.Q + 15) / 16;
  const long long rounds = (groups * a.D + 7) / 8 * 8;
  if (rounds * (a.H / 32) <= device_cus()) l.waves = 2;
  else if (rounds * (a.H / 64) <= device_cus()) l.waves = 4;
  else if (a.D == 2 && (groups + 7) / 8 * 8 * (a.H / 64) <= device_cus()) l.waves = 4, l.per_direction = true;
  else return l;
  l.groups = (int)groups;
  l.hx_bytes = align_up((size_t)2 * a.D * l.groups * 2 * 16 * (a.H + 8) * sizeof(_Float16), 256);
  l.sync_words = align_up((size_t)(a.D * l.groups * (2 + a.H / (16 * l.waves)) + 1) * sizeof(unsigned), 256) / sizeof(unsigned);
  l.bytes = l.hx_bytes + l.sync_words * sizeof(unsigned);
  return l;
}

// Calls f(H, WAVES, PAIRS) with the variant of an H = 256 / 192 launch as std::integral_constant values: the template
// arguments of its kernel (the streamed kernel has no WAVES).
template <class F>
static void with_h256_variant(int H, int waves, bool pairs, F&& f) {
  auto with_pairs = [&](auto HH, auto WW) {
    if (pairs) f(HH, WW, std::integral_constant<int, 2>{});
    else f(HH, WW, std::integral_constant<int, 1>{});
  };
  if (H == 256 && waves == 2) with_pairs(std::integral_constant<int, 256>{}, std::integral_constant<int, 2>{});
  else if (H == 256) with_pairs(std::integral_constant<int, 256>{}, std::integral_constant<int, 4>{});
  else if (waves == 2) with_pairs(std::integral_constant<int, 192>{}, std::integral_constant<int, 2>{});
  else with_pairs(std::integral_constant<int, 192>{}, std::integral_constant<int, 4>{});
}

struct LstmPlan {
  void (*kernel)(LstmK);
  dim3 grid, block;
  size_t lds;
};

// What a (valid) ps_lstm_f32 / ps_lstm_f16x2_f32 launch runs: a function of the arguments and the debug switches alone.
static LstmPlan lstm_plan(const ps_lstm_args& a, bool f16x2) {
  if ((a.H != 64 && a.H != 128) || dbg(PS_DBG_LSTM_SCALAR)) {  // thread = gate row, LS sequences per workgroup
    auto rows = [&](void (*kernel)(LstmK)) {
      return LstmPlan{kernel, dim3((a.Q + LS - 1) / LS, a.N, a.D), dim3((4 * a.H + 63) / 64 * 64), (size_t)5 * a.H * sizeof(f32x4)};
    };
    return a.H <= LSTM_WREG ? rows(lstm_kernel<true>) : rows(lstm_kernel<false>);
  }
  const long long seqs = (long long)a.N * a.Q;
  const bool contig = step_groups(a, true), h64 = a.H == 64, stores_4b = dbg(PS_DBG_LSTM_4B_STORES);
  // 16 sequences per workgroup when there are enough sequences to fill the chip that way (PS_DBG_LSTM_WIDE / _M4 force one)
  const bool wide = dbg(PS_DBG_LSTM_WIDE) ? true : dbg(PS_DBG_LSTM_M4) ? false : (h64 && contig && seqs >= 16 * 256);
  // 4 sequences per workgroup: a multiple of 8 workgroups, see the XCD-aware group order
  const dim3 grid((unsigned)(wide ? (seqs + 15) / 16 : ((seqs + 3) / 4 + 7) / 8 * 8), 1, a.D);
  auto run = [&](void (*kernel)(LstmK)) { return LstmPlan{kernel, grid, dim3(4 * a.H), 0}; };
  if (wide) {
    // whole segments of 20 consecutive frames (DPRNN's intra pass at K = 20): all steps fetched up front
    const bool seg = h64 && contig && a.steps == 20 && !stores_4b;
    if (seg && f16x2) return a.D == 1 ? run(lstm_seg_f16x2_kernel<64, 20, false>) : run(lstm_seg_f16x2_kernel<64, 20, true>);
    if (seg) return a.D == 1 ? run(lstm_seg_kernel<64, 20, false>) : run(lstm_seg_kernel<64, 20, true>);
    if (h64) return contig ? run(lstm_mfma_kernel<64, true>) : run(lstm_mfma_kernel<64, false>);
    return run(lstm_mfma_kernel<128, false>);  // H = 128: the 16-byte group path does not fit the 256-VGPR budget of 8 waves
  }
  if (!h64) return contig ? run(lstm_m4_kernel<128, true>) : run(lstm_m4_kernel<128, false>);
  if (contig) return run(lstm_m4_kernel<64, true>);
  return f16x2 && !stores_4b ? run(lstm_m4_f16x2_kernel) : run(lstm_m4_kernel<64, false>);
}

// ---- entries -------------------------------------------------------------------------------------------------------------
// steps_rows: NULL, or the per-utterance step counts of ps_lstm_rows_f32 (`who`), which runs the thread-per-gate-row kernel's
// ROWS instantiations at every H and takes no state_shift.
static int lstm_launch(const ps_lstm_args* args, void* stream, bool f16x2, const int* steps_rows = nullptr,
                       const char* who = "ps_lstm_f32") {
  if (!args) {
    set_error("%s: null args", who);
    return PS_E_INVALID;
  }
  const ps_lstm_args& a = *args;
  if (!sizes_ok(a) || a.N > 65535) {
    set_error("%s: bad argument (N=%d H=%d D=%d Q=%d steps=%d)", who, a.N, a.H, a.D, a.Q, a.steps);
    return PS_E_INVALID;
  }
  if (4 * a.H > 1024) {
    set_error("%s: hidden size %d > 256 is not supported", who, a.H);
    return PS_E_UNSUPPORTED;
  }
  if (last_frame(a) >= a.ldt) {
    set_error("%s: the last frame %lld lies outside the row (ldt=%d)", who, last_frame(a), a.ldt);
    return PS_E_INVALID;
  }
  if (!states_ok(a)) {
    set_error("%s: ldq=%d < Q=%d", who, a.ldq, a.Q);
    return PS_E_INVALID;
  }
  if (!shift_ok(a, steps_rows ? 0 : 1)) {
    set_error(steps_rows ? "%s: state_shift must be 0" : "%s: state_shift must be 0 or 1", who);
    return PS_E_INVALID;
  }
  if (steps_rows) {
    const dim3 grid((a.Q + LS - 1) / LS, a.N, a.D), block((4 * a.H + 63) / 64 * 64);
    const size_t lds = (size_t)5 * a.H * sizeof(f32x4);
    LaunchTimer timer("lstm", (hipStream_t)stream);
    if (a.H <= LSTM_WREG)
      hipLaunchKernelGGL((lstm_kernel<true, true, const int*>), grid, block, lds, (hipStream_t)stream, LstmK{a}, steps_rows);
    else
      hipLaunchKernelGGL((lstm_kernel<false, true, const int*>), grid, block, lds, (hipStream_t)stream, LstmK{a}, steps_rows);
  } else {
    const LstmPlan p = lstm_plan(a, f16x2);
    LaunchTimer timer("lstm", (hipStream_t)stream);
    hipLaunchKernelGGL(p.kernel, p.grid, p.block, p.lds, (hipStream_t)stream, LstmK{a});
  }
  return launch_status(who);
}

extern "C" int ps_lstm_f32(const ps_lstm_args* args, void* stream) { return lstm_launch(args, stream, false); }
extern "C" int ps_lstm_f16x2_f32(const ps_lstm_args* args, void* stream) { return lstm_launch(args, stream, true); }

extern "C" int ps_lstm_rows_f32(const ps_lstm_args* args, const int* steps_rows, void* stream) {
  if (!steps_rows) {
    set_error("ps_lstm_rows_f32: steps_rows is NULL");
    return PS_E_INVALID;
  }
  return lstm_launch(args, stream, false, steps_rows, "ps_lstm_rows_f32");
}

extern "C" int ps_rnn_f32(const ps_lstm_args* args, int kind, const float* bhn, void* stream) {
  if (!args || (kind != PS_RNN_TANH && kind != PS_RNN_GRU)) {
    set_error("ps_rnn_f32: null args or unknown cell kind %d", kind);
    return PS_E_INVALID;
  }
  const ps_lstm_args& a = *args;
  const int ng = kind == PS_RNN_GRU ? 3 : 1;
  if (!sizes_ok(a) || a.c0 || a.c_last || a.N > 65535 || !shift_ok(a, 0) || (kind == PS_RNN_GRU && !bhn)) {
    set_error("ps_rnn_f32: bad argument (N=%d H=%d D=%d Q=%d steps=%d; no cell states, the GRU needs bhn)", a.N, a.H, a.D, a.Q, a.steps);
    return PS_E_INVALID;
  }
  if (ng * a.H > 1024 || a.H * LS > 1024) {
    set_error("ps_rnn_f32: hidden size %d is not supported (GRU: <= 256, RNN: <= 256)", a.H);
    return PS_E_UNSUPPORTED;
  }
  if (last_frame(a) >= a.ldt || !states_ok(a)) {
    set_error("ps_rnn_f32: a frame lies outside the row (ldt=%d) or ldq=%d < Q=%d", a.ldt, a.ldq, a.Q);
    return PS_E_INVALID;
  }
  LstmK k{a};
  const int rows = ng * a.H > a.H * LS ? ng * a.H : a.H * LS;
  const int threads = (rows + 63) / 64 * 64;
  const size_t lds = (size_t)(a.H + ng * a.H + a.H) * sizeof(f32x4);
  dim3 grid((a.Q + LS - 1) / LS, a.N, a.D);
  {
    LaunchTimer timer("lstm", (hipStream_t)stream);
    if (kind == PS_RNN_GRU)
      hipLaunchKernelGGL((rnn_kernel<2>), grid, dim3(threads), lds, (hipStream_t)stream, k, bhn);
    else
      hipLaunchKernelGGL((rnn_kernel<0>), grid, dim3(threads), lds, (hipStream_t)stream, k, bhn);
  }
  return launch_status("ps_rnn_f32");
}

extern "C" int ps_lstm_fmajor_ok(const ps_lstm_args* args, int ldm) { return args && lstm_fmajor_fits(*args, ldm) ? 1 : 0; }

extern "C" int ps_lstm_fmajor_f16x2_f32(const ps_lstm_args* args, int ldm, void* stream) {
  if (!args || !lstm_fmajor_fits(*args, ldm)) {
    set_error("ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
              "(ps_lstm_fmajor_ok)");
    return args ? PS_E_UNSUPPORTED : PS_E_INVALID;
  }
  const ps_lstm_args& a = *args;
  LstmFm k{a, ldm, g_debug_ablate, (a.Q + 15) / 16, 0};
  k.total = a.N * k.nblk;
  // one workgroup per CU (148 KiB of LDS), the directions side by side; a multiple of 8 for the XCD-aware block order
  int cap = device_cus() / a.D / 8 * 8;
  cap = cap < 8 ? 8 : cap;
  const int want = (k.total + 7) / 8 * 8;
  dim3 grid((unsigned)(want < cap ? want : cap), 1, a.D);
  {
    LaunchTimer timer("lstm", (hipStream_t)stream);
    // (PS_DBG_LSTM_4B_STORES: 4-byte h' stores for consecutive frames too; tests run both)
    if (step_groups(a, false) && !dbg(PS_DBG_LSTM_4B_STORES))
      hipLaunchKernelGGL((lstm_fm_f16x2_kernel<true>), grid, dim3(512), 0, (hipStream_t)stream, k);
    else
      hipLaunchKernelGGL((lstm_fm_f16x2_kernel<false>), grid, dim3(512), 0, (hipStream_t)stream, k);
  }
  return launch_status("ps_lstm_fmajor_f16x2_f32");
}

extern "C" int ps_lstm_fmajor_h256_ok(const ps_lstm_args* args, int ldm) { return args && lstm_h256_fits(*args, ldm) ? 1 : 0; }

extern "C" int ps_lstm_fmajor_h256_f16x2_f32(const ps_lstm_args* args, int ldm, const void* whh_image, const float* acc_scale,
                                             void* stream) {
  if (!args || !whh_image || !acc_scale || ((uintptr_t)whh_image & 15)) {
    set_error("ps_lstm_fmajor_h256_f16x2_f32: null argument or unaligned weight image");
    return PS_E_INVALID;
  }
  if (!lstm_h256_fits(*args, ldm)) {
    set_error("ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H (ps_lstm_fmajor_h256_ok)");
    return PS_E_UNSUPPORTED;
  }
  const ps_lstm_args& a = *args;
  LstmFm256 k{a, ldm, whh_image, {acc_scale[0], a.D > 1 ? acc_scale[1] : acc_scale[0]}};
  if (!(k.up[0] > 0.f) || !(k.up[1] > 0.f)) {
    set_error("ps_lstm_fmajor_h256_f16x2_f32: accumulator scales must be positive");
    return PS_E_INVALID;
  }
  const long long seqs = (long long)a.N * a.Q;
  dim3 grid((unsigned)((seqs + 15) / 16), 1, a.D);
  {
    LaunchTimer timer("lstm", (hipStream_t)stream);
    with_h256_variant(a.H, 0, store_pairs(a), [&](auto H, auto, auto PAIRS) {
      hipLaunchKernelGGL((lstm_fm_h256_kernel<H(), PAIRS()>), grid, dim3(2 * H()), 0, (hipStream_t)stream, k);
    });
  }
  return launch_status("ps_lstm_fmajor_h256_f16x2_f32");
}

extern "C" int ps_lstm_h256_ok(const ps_lstm_args* args) { return args && lstm_h256_f32_fits(*args) ? 1 : 0; }

extern "C" int ps_lstm_h256_f32(const ps_lstm_args* args, const void* whh_image, void* stream) {
  if (!args || !whh_image || ((uintptr_t)whh_image & 15)) {
    set_error("ps_lstm_h256_f32: null argument or unaligned weight image");
    return PS_E_INVALID;
  }
  if (!lstm_h256_f32_fits(*args)) {
    set_error("ps_lstm_h256_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, the gx of 16 sequences' utterances below "
              "2 GiB (ps_lstm_h256_ok)");
    return PS_E_UNSUPPORTED;
  }
  const ps_lstm_args& a = *args;
  LstmH256F32 k{a, whh_image, h256_f32_span(a)};
  const long long seqs = (long long)a.N * a.Q;
  dim3 grid((unsigned)((seqs + 15) / 16), 1, a.D);
  {
    LaunchTimer timer("lstm", (hipStream_t)stream);
    if (a.H == 256) hipLaunchKernelGGL((lstm_h256_f32_kernel<256>), grid, dim3(512), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL((lstm_h256_f32_kernel<192>), grid, dim3(384), 0, (hipStream_t)stream, k);
  }
  return launch_status("ps_lstm_h256_f32");
}

extern "C" size_t ps_lstm_fmajor_coop_workspace_bytes(const ps_lstm_args* args, int ldm) { return args ? coop_layout(*args, ldm).bytes : 0; }

extern "C" int ps_lstm_fmajor_coop_f16x2_f32(const ps_lstm_args* args, int ldm, const void* whh_image, const float* acc_scale,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!args || !whh_image || !acc_scale || !workspace || ((uintptr_t)whh_image & 15) || ((uintptr_t)workspace & 255)) {
    set_error("ps_lstm_fmajor_coop_f16x2_f32: null argument, unaligned weight image or workspace (256 bytes)");
    return PS_E_INVALID;
  }
  const ps_lstm_args& a = *args;
  const CoopLayout l = coop_layout(a, ldm);
  if (!l.waves) {
    set_error("ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most %d / (D * H / 64) groups of 16 "
              "sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)", device_cus());
    return PS_E_UNSUPPORTED;
  }
  if (workspace_bytes < l.bytes) {
    set_error("ps_lstm_fmajor_coop_f16x2_f32: workspace too small (%zu < %zu)", workspace_bytes, l.bytes);
    return PS_E_INVALID;
  }
  LstmCoop k{a, ldm, whh_image, {acc_scale[0], a.D > 1 ? acc_scale[1] : acc_scale[0]}, (_Float16*)workspace,
             (unsigned*)((char*)workspace + l.hx_bytes), l.groups, dbg(PS_DBG_COOP_AGENT_FENCES) ? 0 : 1,
             dbg(PS_DBG_COOP_SCATTER) ? 1 : 0, dbg(PS_DBG_COOP_SABOTAGE) ? 1 : 0, 0, a.D, g_debug_ablate};
  if (!(k.up[0] > 0.f) || !(k.up[1] > 0.f)) {
    set_error("ps_lstm_fmajor_coop_f16x2_f32: accumulator scales must be positive");
    return PS_E_INVALID;
  }
  hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, k.sync, (int)l.sync_words);
  {
    LaunchTimer timer("lstm", (hipStream_t)stream);
    // clusters (direction, group) in rounds of 8, one per XCD; H / (16 waves) slices each
    for (int d0 = 0; d0 < (l.per_direction ? a.D : 1); ++d0) {
      if (l.per_direction) k.d0 = d0, k.nd = 1;
      dim3 grid((unsigned)((k.nd * l.groups + 7) / 8 * (a.H / (16 * l.waves)) * 8));
      with_h256_variant(a.H, l.waves, store_pairs(a), [&](auto H, auto WAVES, auto PAIRS) {
        hipLaunchKernelGGL((lstm_coop_kernel<H(), WAVES(), PAIRS()>), grid, dim3(64 * WAVES()), 0, (hipStream_t)stream, k);
      });
    }
  }
  return launch_status("ps_lstm_fmajor_coop_f16x2_f32");
}
