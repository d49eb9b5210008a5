// Batches of utterances of unequal length through the Conv-TasNet masker: row n of [N][R][ldt] holds t_rows[n] <= T valid
// frames and anything at all behind them (the features of the junk that follows a short utterance in its row, NaN included).
//
// In a TCN block frames meet each other in three places only -- the statistics of the global norms, the taps of the depthwise
// convolution and the decoder's overlap-add; the three 1x1 GEMMs with their prologues, the embedding bias and the residual are
// column-wise.  So the ragged masker keeps ps_conv1x1_f32 over all T frames, untouched (a column t >= t_rows[n] may hold
// anything as long as nothing reads it as data), and the kernels here stand where frames meet:
//   ps_ragged_stats_f32    the (sum, sum of squares) partials of a GEMM's output over t < t_rows[n] only,
//   ps_dwconv_ragged_f32   ps_dwconv_f32 with a per-row frame limit: a = prologue(x) is 0 outside [0, t_rows[n]),
//   ps_zero_tail_f32       0.0 behind a per-row limit: features and mask logits in front of the decoder, the waveform after it,
//   ps_align_rows_f32      the clean reference of a score, aligned to each row's valid output length (behind the decoder),
//   ps_conv_tasnet_ragged_f32   the block loop of ps_conv_tasnet_f32 over them, always in the exact-fp32 arithmetic.
// Both statistics kernels scale their partials by count_full / (R * t_rows[n]): the consumers divide the sums by the launch-wide
// ps_prologue.count = R * T (load_norm_scalars), which then gives mean = S1 / (R T_n) and var = S2 / (R T_n) - mean^2.
#include <type_traits>

#include "ps_common.h"

namespace ps {

// ---- statistics of [N][R][ldt] over t < t_rows[n] ----------------------------------------------------------------------------
// Workgroup (p, n) sums rows p, p + parts, ... of utterance n with 16-byte loads, in fp64, in a fixed order (no atomics), and
// writes slot p; a slot without rows holds 0, because the consumers add up every slot.
__global__ __launch_bounds__(256) void ragged_stats_kernel(const float* __restrict__ y, const int* __restrict__ t_rows,
                                                           double* __restrict__ ostats, int R, int T, int ldt, int parts,
                                                           double count_full) {
  __shared__ double red[8];
  const int p = blockIdx.x, n = blockIdx.y;
  const int tn = row_limit(t_rows, n, T);
  const int nv = (tn + 3) / 4;
  double s = 0.0, q = 0.0;
  for (int r = p; r < R; r += parts) {
    const float* row = y + ((size_t)n * R + r) * ldt;
#pragma unroll 4
    for (int i = threadIdx.x; i < nv; i += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * i);  // (4 i < tn <= T <= ldt, ldt a multiple of 4)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = 4 * i + e < tn ? (double)v[e] : 0.0;  // a select: what lies behind the row's end may be a NaN
        s += d;
        q += d * d;
      }
    }
  }
  block_sum2(s, q, red);
  if (threadIdx.x == 0) {
    const double scale = tn > 0 ? count_full / ((double)R * (double)tn) : 0.0;
    double* dst = ostats + ((size_t)n * parts + p) * 2;
    dst[0] = s * scale;
    dst[1] = q * scale;
  }
}

// ---- 0.0 behind a per-row limit ------------------------------------------------------------------------------------------------
// Workgroup (r, n) stores zeros at columns [limit[n], ld) of row r; nothing is loaded.  VEC: 16-byte stores from the first
// multiple of 4 at or behind the limit (rows of a multiple of 4 floats at a 16-byte aligned base).
template <bool VEC>
__global__ __launch_bounds__(256) void zero_tail_kernel(float* __restrict__ x, const int* __restrict__ limit, int R, int ld) {
  const int r = blockIdx.x, n = blockIdx.y;
  const int lim = row_limit(limit, n, ld);
  float* row = x + ((size_t)n * R + r) * ld;
  if constexpr (VEC) {
    const int up = (lim + 3) / 4 * 4;  // <= ld
    if ((int)threadIdx.x < up - lim) row[lim + threadIdx.x] = 0.f;
    for (int t = up + 4 * threadIdx.x; t < ld; t += 1024) *reinterpret_cast<f32x4*>(row + t) = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (int t = lim + threadIdx.x; t < ld; t += 256) row[t] = 0.f;
  }
}

// ---- a reference aligned to each row's valid output length -----------------------------------------------------------------------
// _align_waveform's rule (base_nn.py:398-412) per row: with a = a_len[n] valid output samples and b = b_len[n] reference samples,
// d = max(0, a - b): out[n][s] = ref[n][s - d] on d <= s < a (a shorter reference is left-padded with zeros, a longer one is
// cut) and 0.0 everywhere else.  s - d < min(a, b) <= b: no load leaves the reference's valid samples, and what lies behind them
// is never loaded.  The source index is shifted by d, so the loads are dwords; VEC: one 16-byte store per thread (rows of a
// multiple of 4 floats at a 16-byte aligned base), otherwise four coalesced dword stores.
template <bool VEC>
__global__ __launch_bounds__(256) void align_rows_kernel(const float* __restrict__ ref, float* __restrict__ out,
                                                         const int* __restrict__ a_len, const int* __restrict__ b_len, int L_out,
                                                         int L_ref, int ldr) {
  const int n = blockIdx.y;
  const int a = row_limit(a_len, n, L_out), b = row_limit(b_len, n, L_ref);
  const int d = a > b ? a - b : 0;
  const float* src = ref + (size_t)n * ldr;
  float* dst = out + (size_t)n * L_out;
  if constexpr (VEC) {
    const int s = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (s >= L_out) return;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (s + e >= d && s + e < a) ? src[s + e - d] : 0.f;
    *reinterpret_cast<f32x4*>(dst + s) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int s = blockIdx.x * 1024 + e * 256 + threadIdx.x;
      if (s < L_out) dst[s] = (s >= d && s < a) ? src[s - d] : 0.f;
    }
  }
}

// ---- depthwise dilated convolution with a per-row frame limit --------------------------------------------------------------------
// dwconv_kernel (dwconv.hip) with T_n = t_rows[n] in the place of T wherever T says where an utterance ends: a workgroup owns
// RD_ROWS channels x RD_FRAMES frames and walks them RD_RB rows at a time; each row segment [t0 - left, t0 + RD_FRAMES + right)
// is loaded once with coalesced 16-byte loads (pieces that begin at or behind T_n are not loaded), normalised + activated once
// per element, set to 0 outside [0, T_n) -- by a select per element, so that a NaN behind the row's end stays there -- and
// written to LDS; the taps are LDS reads.  The loads of row batch b + 1 are in flight while batch b is consumed.  y is 0 on
// [T_n, T); a tile that lies at or behind T_n stores its zeros and its empty statistics slot without loading anything.  The
// statistics are gathered in fp64 over t < T_n.
constexpr int RD_ROWS = 16;
constexpr int RD_FRAMES = 1024;  // 256 threads x 4
constexpr int RD_MAXP = 8;
constexpr int RD_RB = 4;            // rows staged together
constexpr int RD_MAXHALO = 1024;    // (P-1)*dilation + 8 frames of halo the LDS image can hold ...
constexpr int RD_SMALLHALO = 288;   // ... and in the small-halo build (P = 3, dilation <= 128: 21 KiB of LDS instead of 32)

struct RaggedDwArgs {
  const float* x;
  const float* w;
  const float* b;
  float* y;
  const int* t_rows;
  double* ostats;
  ps_prologue pro;
  int H, T, ldt, P, dilation, left;
  double count_full;
};

// P > 0: compile-time tap count; P == 0: run-time taps.  ALIGNED: every tap offset is a multiple of 4 frames.
template <int P, bool ALIGNED, int HALO>
__global__ __launch_bounds__(256) void dwconv_ragged_kernel(RaggedDwArgs a) {
  constexpr int SEG = RD_FRAMES + HALO;
  __shared__ __attribute__((aligned(16))) float seg[RD_RB][SEG];
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const int n = blockIdx.z;
  const int h0 = blockIdx.y * RD_ROWS;
  const int t0 = blockIdx.x * RD_FRAMES;
  const int t = t0 + tid * 4;
  const int tn = row_limit(a.t_rows, n, a.T);
  double* const slot = a.ostats ? a.ostats + ((size_t)n * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x) * 2
                                : nullptr;
  if (t0 >= tn) {  // (uniform) the whole tile lies behind the utterance
    if (t < a.T)
      for (int r = 0; r < RD_ROWS && h0 + r < a.H; ++r)
        *reinterpret_cast<f32x4*>(a.y + ((size_t)n * a.H + h0 + r) * a.ldt + t) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (slot && tid == 0) slot[0] = slot[1] = 0.0;
    return;
  }
  const int np = P > 0 ? P : a.P;
  const int halo = (np - 1) * a.dilation;  // left + right
  // segment origin in frames, rounded down to a multiple of 4 so that every staging load is 16-byte aligned
  const int lpad = (a.left + 3) / 4 * 4;
  const int org = t0 - lpad;               // frame of seg[.][0]
  const int shift = lpad - a.left;         // tap j of output frame f reads seg[f - t0 + j*dilation + shift]
  const int nvec = RD_FRAMES / 4 + (lpad + halo - a.left + 3) / 4;  // vectors that can be touched: <= SEG / 4 (launcher)

  const bool has_norm = a.pro.norm != PS_NORM_NONE;
  const bool has_prelu = a.pro.prelu != 0;
  const float slope = has_prelu ? a.pro.slope[0] : 1.f;
  const bool slope01 = slope >= 0.f && slope <= 1.f;

  double dsum = 0.0, dsq = 0.0;
  const int i1 = tid + 256;  // second vector index (halo part): only the first (nvec - 256) threads
  f32x4 v[2][RD_RB][2];
  auto load_batch = [&](int r0, auto q_c) {
    constexpr int q = decltype(q_c)::value;
#pragma unroll
    for (int r = 0; r < RD_RB; ++r) {
      const int h = h0 + r0 + r;
      const size_t row = ((size_t)n * a.H + (h < a.H ? h : a.H - 1)) * a.ldt;
      const int f0 = org + tid * 4, f1 = org + i1 * 4;
      v[q][r][0] = (f0 >= 0 && f0 < tn) ? *reinterpret_cast<const f32x4*>(a.x + row + f0) : f32x4{0.f, 0.f, 0.f, 0.f};
      v[q][r][1] = (i1 < nvec && f1 >= 0 && f1 < tn) ? *reinterpret_cast<const f32x4*>(a.x + row + f1)
                                                      : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  static_assert(RD_ROWS / RD_RB == 4, "four row batches, unrolled below");
  using q0 = std::integral_constant<int, 0>;
  using q1 = std::integral_constant<int, 1>;
  const int nb = (a.H - h0 + RD_RB - 1) / RD_RB;  // batches that hold rows (uniform)
  load_batch(0, q0{});
  if (nb > 1) load_batch(RD_RB, q1{});
  float gam[RD_ROWS], bet[RD_ROWS];
#pragma unroll
  for (int r = 0; r < RD_ROWS; ++r) {
    const int hc = h0 + r < a.H ? h0 + r : a.H - 1;
    gam[r] = has_norm ? a.pro.gamma[hc] : 1.f;
    bet[r] = has_norm ? a.pro.beta[hc] : 0.f;
  }
  const NormScalars ns = load_norm_scalars(a.pro, n, red);  // (behind the first loads)
  auto process_batch = [&](auto r0_c, auto q_c) {
    constexpr int r0 = decltype(r0_c)::value;
    constexpr int qb = decltype(q_c)::value;
    // ---- transform once, zero outside [0, T_n), write LDS ----------------------------------------------------------------------
#pragma unroll
    for (int r = 0; r < RD_RB; ++r) {
      const float sc = has_norm ? gam[r0 + r] * ns.rstd : 1.f;
      const float sh = bet[r0 + r] - ns.mean * sc;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int idx = q == 0 ? tid : i1;
        if (q == 1 && idx >= nvec) continue;
        const int f = org + idx * 4;
        f32x4 u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float z = v[qb][r][q][e] * sc + sh;
          if (has_prelu) z = slope01 ? fmaxf(z, slope * z) : prelu(z, slope);
          u[e] = z;
        }
        if (!(f >= 0 && f + 3 < tn)) {  // edge vectors only: the conv's zero padding, applied AFTER norm + PReLU, per element
#pragma unroll
          for (int e = 0; e < 4; ++e) u[e] = (f + e >= 0 && f + e < tn) ? u[e] : 0.f;
        }
        *reinterpret_cast<f32x4*>(&seg[r][idx * 4]) = u;
      }
    }
    __syncthreads();
    // ---- taps from LDS, bias, statistics, store ----------------------------------------------------------------------------------
    if (t < a.T) {
#pragma unroll
      for (int r = 0; r < RD_RB; ++r) {
        const int h = h0 + r0 + r;
        if (h < a.H) {
          f32x4 out{0.f, 0.f, 0.f, 0.f};
          if (t < tn) {
            const float bias = a.b ? a.b[h] : 0.f;
            out = f32x4{bias, bias, bias, bias};
            const float* sp = &seg[r][tid * 4 + shift];
            if constexpr (P > 0) {
#pragma unroll
              for (int j = 0; j < P; ++j) {
                const float wj = a.w[h * P + j];
                f32x4 s;
                if constexpr (ALIGNED) {
                  s = *reinterpret_cast<const f32x4*>(sp + j * a.dilation);
                } else {
#pragma unroll
                  for (int e = 0; e < 4; ++e) s[e] = sp[j * a.dilation + e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) out[e] += wj * s[e];
              }
            } else {
              for (int j = 0; j < np; ++j) {
                const float wj = a.w[h * np + j];
#pragma unroll
                for (int e = 0; e < 4; ++e) out[e] += wj * sp[j * a.dilation + e];
              }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              out[e] = t + e < tn ? out[e] : 0.f;  // y is 0 on [T_n, T); the zeros add nothing to the sums below
              dsum += (double)out[e];
              dsq += (double)out[e] * (double)out[e];
            }
          }
          *reinterpret_cast<f32x4*>(a.y + ((size_t)n * a.H + h) * a.ldt + t) = out;
        }
      }
    }
    __syncthreads();  // the next batch overwrites the LDS image
  };
  process_batch(q0{}, q0{});
  if (nb > 1) {
    if (nb > 2) load_batch(2 * RD_RB, q0{});
    process_batch(std::integral_constant<int, RD_RB>{}, q1{});
    if (nb > 2) {
      if (nb > 3) load_batch(3 * RD_RB, q1{});
      process_batch(std::integral_constant<int, 2 * RD_RB>{}, q0{});
      if (nb > 3) process_batch(std::integral_constant<int, 3 * RD_RB>{}, q1{});
    }
  }
  if (slot) {
    block_sum2(dsum, dsq, red);
    if (tid == 0) {
      const double scale = a.count_full / ((double)a.H * (double)tn);  // (tn > t0 >= 0)
      slot[0] = dsum * scale;
      slot[1] = dsq * scale;
    }
  }
}

// ---- checks ------------------------------------------------------------------------------------------------------------------------
static int rows_check(const char* who, const void* x, const int* lim, int N, int R, int T, int ldt) {
  if (!x || !lim || N <= 0 || N > 65535 || R <= 0 || T <= 0) {  // (N is a grid's y or z extent)
    set_error("%s: null pointer or a size outside its range (N=%d in 1 .. 65535, rows=%d, T=%d)", who, N, R, T);
    return PS_E_INVALID;
  }
  if (ldt < T || ldt % kTileT != 0 || ((uintptr_t)x & 15)) {
    set_error("%s: ldt=%d must be a multiple of %d >= T=%d and pointers 16-byte aligned", who, ldt, kTileT, T);
    return PS_E_ALIGN;
  }
  return 0;
}

static int dwconv_ragged_check(const float* x, const float* w, const float* y, const int* t_rows, int N, int H, int T, int ldt,
                               int P, int dilation, int left, const ps_prologue* pro, const double* ostats, double count_full) {
  const char* who = "ps_dwconv_ragged_f32";
  if (!w || !y || P <= 0 || P > RD_MAXP || dilation <= 0 || left < 0) {
    set_error("%s: bad argument (P=%d dilation=%d left=%d)", who, P, dilation, left);
    return PS_E_INVALID;
  }
  if (const int rc = rows_check(who, x, t_rows, N, H, T, ldt)) return rc;
  if ((uintptr_t)y & 15) {
    set_error("%s: y must be 16-byte aligned", who);
    return PS_E_ALIGN;
  }
  if (x == y) {
    set_error("%s: y must not alias x (a tile reads its neighbours' frames)", who);
    return PS_E_INVALID;
  }
  if (left > (P - 1) * dilation) {
    set_error("%s: left=%d exceeds the receptive field (P-1)*dilation=%d", who, left, (P - 1) * dilation);
    return PS_E_INVALID;
  }
  if ((P - 1) * dilation + 8 > RD_MAXHALO) {
    set_error("%s: (P-1)*dilation=%d exceeds the %d-frame halo the LDS tile holds", who, (P - 1) * dilation, RD_MAXHALO - 8);
    return PS_E_UNSUPPORTED;
  }
  if (ostats && !(count_full > 0.0)) {
    set_error("%s: the statistics need count_full > 0 (the count the consumer's prologue divides by)", who);
    return PS_E_INVALID;
  }
  if (const int rc = check_prologue(who, pro)) return rc;
  if (pro && pro->norm != PS_NORM_NONE && (!pro->gamma || !pro->beta)) {
    set_error("%s: norm prologue needs gamma/beta", who);
    return PS_E_INVALID;
  }
  return 0;
}

// The driver's checks: those of the masker's other entries that apply (check_stack), and what only this entry needs
static int ragged_check(const ps_tcn_block* blocks, int n_blocks, const float* x_in, const float* x_out, const float* dvec,
                        int N, int T, int ldt, const int* t_rows, const void* workspace, size_t workspace_bytes) {
  if (const int rc = check_stack(blocks, n_blocks, x_in, x_out, N, T, ldt, workspace, workspace_bytes)) return rc;
  if (!t_rows) {
    set_error("ps_conv_tasnet_ragged_f32: t_rows is NULL");
    return PS_E_INVALID;
  }
  for (int i = 0; i < n_blocks; ++i) {
    const ps_tcn_block& b = blocks[i];
    if (b.in_embed_w && !dvec) {
      set_error("ps_conv_tasnet_f32: block expects an embedding (E=%d) but dvec is NULL", b.E);
      return PS_E_INVALID;
    }
    if (!b.in_wt || !b.pw_wt || !b.out_wt || !b.dw_w) {
      set_error("ps_conv_tasnet_ragged_f32: block %d lacks the fp32 weights in_wt / dw_w / pw_wt / out_wt", i);
      return PS_E_INVALID;
    }
    if (b.P > RD_MAXP || (b.P - 1) * b.dilation + 8 > RD_MAXHALO) {
      set_error("ps_conv_tasnet_ragged_f32: block %d: P=%d dilation=%d is outside ps_dwconv_ragged_f32", i, b.P, b.dilation);
      return PS_E_UNSUPPORTED;
    }
  }
  return 0;
}

// One block: launch_block (abi.hip) on the exact-fp32 GEMM entry without its statistics epilogue, the statistics of the two
// GEMM outputs from ps_ragged_stats_f32 and the depthwise stage from ps_dwconv_ragged_f32
static int ragged_block(const ps_tcn_block& b, const float* x_in, float* x_out, const float* dvec, int embed_norm, int N, int T,
                        int ldt, const int* t_rows, const TasnetWs& w, void* stream) {
  int rc;
  const double count = (double)b.H * (double)T;
  const int dw_parts = ps_dwconv_stats_parts(b.H, T);
  const float* bias_n = b.in_embed_w ? w.bias_n : nullptr;
  if (bias_n && (rc = ps_embed_bias_f32(dvec, b.in_embed_w, w.bias_n, N, b.E, b.H, embed_norm, stream))) return rc;
  if ((rc = ps_conv1x1_f32(x_in, b.in_wt, w.y1, N, b.C, b.H, T, ldt, nullptr, nullptr, bias_n, nullptr, nullptr, stream))) return rc;
  if (b.in_norm == PS_NORM_GLOBAL && (rc = ps_ragged_stats_f32(w.y1, t_rows, w.s1, N, b.H, T, ldt, w.parts, count, stream)))
    return rc;

  const ps_prologue p1 = norm_prelu(b.in_norm, w.s1, w.parts, count, b.in_gamma, b.in_beta, b.in_slope);
  rc = ps_dwconv_ragged_f32(w.y1, b.dw_w, b.dw_b, w.y2, t_rows, N, b.H, T, ldt, b.P, b.dilation, dw_left(b.P, b.dilation, b.causal),
                            &p1, b.dw_norm == PS_NORM_GLOBAL ? w.s2 : nullptr, count, stream);
  if (rc) return rc;

  const ps_prologue p2 = norm_prelu(b.dw_norm, w.s2, dw_parts, count, b.dw_gamma, b.dw_beta, b.dw_slope);
  if ((rc = ps_conv1x1_f32(w.y2, b.pw_wt, w.y3, N, b.H, b.H, T, ldt, &p2, b.pw_b, nullptr, nullptr, nullptr, stream))) return rc;
  if (b.pw_norm == PS_NORM_GLOBAL && (rc = ps_ragged_stats_f32(w.y3, t_rows, w.s3, N, b.H, T, ldt, w.parts, count, stream)))
    return rc;

  const ps_prologue p3 = norm_prelu(b.pw_norm, w.s3, w.parts, count, b.pw_gamma, b.pw_beta, b.pw_slope);
  return ps_conv1x1_f32(w.y3, b.out_wt, x_out, N, b.H, b.C, T, ldt, &p3, b.out_b, nullptr, x_in, nullptr, stream);
}

}  // namespace ps

// ---- entries -----------------------------------------------------------------------------------------------------------------------
extern "C" int ps_ragged_stats_f32(const float* y, const int* t_rows, double* ostats, int N, int R, int T, int ldt, int parts,
                                   double count_full, void* stream) {
  using namespace ps;
  if (const int rc = rows_check("ps_ragged_stats_f32", y, t_rows, N, R, T, ldt)) return rc;
  if (!ostats || parts <= 0 || !(count_full > 0.0)) {
    set_error("ps_ragged_stats_f32: ostats, parts > 0 and count_full > 0 are needed (parts=%d)", parts);
    return PS_E_INVALID;
  }
  {
    LaunchTimer timer("ragged_stats", (hipStream_t)stream);
    hipLaunchKernelGGL(ragged_stats_kernel, dim3(parts, N), dim3(256), 0, (hipStream_t)stream, y, t_rows, ostats, R, T, ldt, parts,
                       count_full);
  }
  return launch_status("ps_ragged_stats_f32");
}

extern "C" int ps_zero_tail_f32(float* x, const int* limit, int N, int R, int ld, void* stream) {
  using namespace ps;
  if (!x || !limit || N <= 0 || N > 65535 || R <= 0 || ld <= 0) {
    set_error("ps_zero_tail_f32: null pointer or a size outside its range (N=%d in 1 .. 65535, rows=%d, ld=%d)", N, R, ld);
    return PS_E_INVALID;
  }
  {
    LaunchTimer timer("zero_tail", (hipStream_t)stream);
    if (ld % 4 == 0 && !((uintptr_t)x & 15))
      hipLaunchKernelGGL(zero_tail_kernel<true>, dim3(R, N), dim3(256), 0, (hipStream_t)stream, x, limit, R, ld);
    else
      hipLaunchKernelGGL(zero_tail_kernel<false>, dim3(R, N), dim3(256), 0, (hipStream_t)stream, x, limit, R, ld);
  }
  return launch_status("ps_zero_tail_f32");
}

extern "C" int ps_align_rows_f32(const float* ref, float* out, const int* a_len, const int* b_len, int N, int L_out, int L_ref,
                                 int ldr, void* stream) {
  using namespace ps;
  if (!ref || !out || !a_len || !b_len || N <= 0 || N > 65535 || L_out <= 0 || L_ref <= 0 || ldr < L_ref) {
    set_error("ps_align_rows_f32: null pointer or a size outside its range (N=%d in 1 .. 65535, L_out=%d, L_ref=%d, ldr=%d)", N,
              L_out, L_ref, ldr);
    return PS_E_INVALID;
  }
  if (ref == out) {
    set_error("ps_align_rows_f32: out must not alias ref (a row is read at a shifted index)");
    return PS_E_INVALID;
  }
  {
    LaunchTimer timer("align_rows", (hipStream_t)stream);
    const dim3 grid((L_out + 1023) / 1024, N);
    if (L_out % 4 == 0 && !((uintptr_t)out & 15))
      hipLaunchKernelGGL(align_rows_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, ref, out, a_len, b_len, L_out, L_ref, ldr);
    else
      hipLaunchKernelGGL(align_rows_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, ref, out, a_len, b_len, L_out, L_ref,
                         ldr);
  }
  return launch_status("ps_align_rows_f32");
}

extern "C" int ps_dwconv_ragged_f32(const float* x, const float* w, const float* b, float* y, const int* t_rows, int N, int H,
                                    int T, int ldt, int P, int dilation, int left, const ps_prologue* pro, double* ostats,
                                    double count_full, void* stream) {
  using namespace ps;
  if (const int rc = dwconv_ragged_check(x, w, y, t_rows, N, H, T, ldt, P, dilation, left, pro, ostats, count_full)) return rc;
  const RaggedDwArgs a{x, w, b, y, t_rows, ostats, pro ? *pro : ps_prologue{}, H, T, ldt, P, dilation, left, count_full};
  const dim3 grid((T + RD_FRAMES - 1) / RD_FRAMES, (H + RD_ROWS - 1) / RD_ROWS, N);
  if (ostats && (int)(grid.x * grid.y) != ps_dwconv_stats_parts(H, T)) {  // (one slot per workgroup, as ps_dwconv_f32's)
    set_error("ps_dwconv_ragged_f32: the kernel's tiles do not match ps_dwconv_stats_parts");
    return PS_E_UNSUPPORTED;
  }
  const hipStream_t st = (hipStream_t)stream;
  const bool aligned = dilation % 4 == 0 && left % 4 == 0, small = (P - 1) * dilation + 8 <= RD_SMALLHALO;
  {
    LaunchTimer timer("dwconv_ragged", st);
    if (P != 3)
      hipLaunchKernelGGL((dwconv_ragged_kernel<0, false, RD_MAXHALO>), grid, dim3(256), 0, st, a);
    else if (aligned && small)
      hipLaunchKernelGGL((dwconv_ragged_kernel<3, true, RD_SMALLHALO>), grid, dim3(256), 0, st, a);
    else if (aligned)
      hipLaunchKernelGGL((dwconv_ragged_kernel<3, true, RD_MAXHALO>), grid, dim3(256), 0, st, a);
    else if (small)
      hipLaunchKernelGGL((dwconv_ragged_kernel<3, false, RD_SMALLHALO>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((dwconv_ragged_kernel<3, false, RD_MAXHALO>), grid, dim3(256), 0, st, a);
  }
  return launch_status("ps_dwconv_ragged_f32");
}

extern "C" int ps_conv_tasnet_ragged_f32(const ps_tcn_block* blocks, int n_blocks, const float* x_in, float* x_out,
                                         const float* dvec, int embed_norm, int N, int T, int ldt, const int* t_rows,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  using namespace ps;
  if (const int rc = ragged_check(blocks, n_blocks, x_in, x_out, dvec, N, T, ldt, t_rows, workspace, workspace_bytes)) return rc;
  const TasnetWs w = carve(workspace, N, blocks[0].C, blocks[0].H, T);
  // block 0 reads the caller's input and writes x_out; later blocks update x_out in place
  for (int i = 0; i < n_blocks; ++i)
    if (const int rc = ragged_block(blocks[i], i == 0 ? x_in : x_out, x_out, dvec, embed_norm, N, T, ldt, t_rows, w, stream))
      return rc;
  return 0;
}
