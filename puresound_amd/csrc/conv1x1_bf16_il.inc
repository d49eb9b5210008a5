// ---- "interleaved" persistent variant (included by conv1x1_bf16.hip) ----------------------------------------------------
// One persistent 512-thread workgroup per CU; the two halves (waves 0-3 / 4-7, one wave of each per SIMD) own the two
// 256 x 128 tiles of a 256 (m) x 256 (t) supertile and share the weight tiles, as in conv1x1_bf16_pp_kernel.  What is
// different: there is ONE workgroup barrier per K-step interval, and a wave does not run its 48 MFMAs and its staging
// code as two separate bursts.
//
// What the measurements said (tools/stamp_bf16.py, tools/sweep_stamps.sh; cycles per K-step interval, 3072 = the two
// halves' 96 MFMAs back to back on a SIMD):
//   * ping-pong kernel: 2 x 2650.  Every phase opens with 500-630 cycles of exposed fragment reads (the activation slot
//     is complete only at the barrier that opens the phase) and the DMA issue sits inside the MFMA stream.
//   * one barrier, halves staggered as [M | S] / [S | M] bursts (an intermediate form of this file): 4900.  Next to a
//     partner that streams MFMAs back to back a staging instruction gets ONE issue slot per MFMA -- 45 instructions =
//     1800 cycles, 760 with the MFMAs ablated -- so a wave's own path M + S bounds the interval whatever its partner does.
//   * An MFMA's own wave, however, issues several instructions in the 32 cycles its MFMA occupies the pipe.  So here the
//     step's other work -- DMA issue, transform / split of the activations of step i+2, LDS writes -- is cut into
//     chunks and each chunk follows a group of four of the wave's own MFMAs: 4500-4700.  What is left, by ablation
//     (wall time of the in_conv shape): the DMA instructions 20 % (one per slot: the next piece's M0 write waits for
//     the piece before it, so three back to back stall the wave and its MFMAs), the staging arithmetic 3 %, the
//     fragment reads / barrier at the interval boundary the rest.
//
//   * Later finding (tools/probe/dma_cost_probe.hip, profiles/r02_mfma_power_probe.txt): most of what the ablations
//     priced as "DMA issue" is the clock.  The board sits at its 1400 W cap under this kernel; a pure MFMA stream of
//     this shape is 99 % busy in cycles with or without the DMA pieces, but holds 1.65 GHz alone and 1.25 GHz next to
//     4 TB/s of HBM traffic.  Removing stall cycles without removing work leaves the wall time where it was -- which
//     is why the three-product fp16 split (PLANES = 2, half the matrix-pipe work) is the default arithmetic.
//
// One barrier is enough because
//   * activations are staged TWO steps ahead into a two-slot ring per half: slot (i+2)&1 is written in interval i, its
//     previous content (step i) went into registers at the end of interval i-1;
//   * the B fragments of step i+1 replace those of step i plane by plane behind each plane's last MFMA of the step and
//     stay in registers across the barrier;
//   * weights: two slots; slot i&1 is read during interval i (both halves), A(i+1) is DMA'd into the other slot during
//     interval i (each half its share) and has landed, by a counted wait, before barrier i;
//   * raw activations: three slots per half; x(i+4) is issued in interval i into the slot S(i+1) emptied in interval
//     i-1 and has two intervals to land (it is waited for at the end of interval i+1).
// Every wave issues A(i+1) then x(i+4) in interval i, so "vmcnt(2)" at the end of the interval means "everything but
// x(i+4)".  A tile's drain follows the barrier that ends its last step.
#ifndef IL2_NA
#define IL2_NA 3
#endif
#ifndef IL2_D
#define IL2_D 4
#endif
template <int PLANES>
struct IlLds {
  static constexpr int A_SLOT = PLANES * XB_M * XB_K * 2;  // 8 KiB per plane
  static constexpr int B_SLOT = PLANES * XB_T * XB_K * 2;  // 4 KiB per plane
  // ring depths.  A(g + DA) and x(g + DX) are issued in interval g: DA = NA - 1, DX = D + 1 (see the wait count below).
  // PLANES = 2 (the HBM-bound arithmetic) has LDS left for a deeper queue: more bytes in flight per CU.
  static constexpr int NA = PLANES == 2 ? IL2_NA : 2;      // weight ring slots
  static constexpr int D = PLANES == 2 ? IL2_D : 3;        // raw activation ring slots per half
  static constexpr int NB = 2;                             // split activation slots per half
  static constexpr int RAW = XB_K * XB_T * 4;
  static constexpr int OFF_RAW = NA * A_SLOT;              // [half][D][RAW]
  static constexpr int OFF_B = OFF_RAW + 2 * D * RAW;      // [half][NB][B_SLOT]
  static constexpr int OFF_TAB = OFF_B + 2 * NB * B_SLOT;  // [PP_MAXU][sc[512] | sh[512]] floats
  static constexpr int OFF_BIAS = OFF_TAB + PP_MAXU * 1024 * 4;
  static constexpr int TOTAL = OFF_BIAS + 4 * XB_M * 4;    // PLANES = 3: 156 KiB
};
static_assert(IlLds<3>::TOTAL <= 160 * 1024, "one workgroup per CU");
#ifndef IL_PRIO1
#define IL_PRIO1 1  // static priority of half 1 (the younger waves) in the main loop
#endif
// cache-policy bits (buffer instruction aux: 1 = sc0, 2 = nt, 16 = sc1) of the streamed activations, the tile stores and
// the residual loads -- experiment hooks, 0 = default policy (nt / sc0 / sc1 on any of the three: no change beyond noise)
#ifndef IL_X_AUX
#define IL_X_AUX 0
#endif
#ifndef IL_ST_AUX
#define IL_ST_AUX 0
#endif
#ifndef IL_RS_AUX
#define IL_RS_AUX 0
#endif
#ifndef IL_F16_NQ
#define IL_F16_NQ 3  // fp16x2: MFMA groups (side-work slots) per row block: 3 (pairs of MFMAs) or 1 (all six)
#endif
// XB / YB: the activation rows of x / y are bf16 in HBM (the hidden maps of a TCN block in the "bf16" arithmetic,
// PLANES = 1): half the DMA pieces per K-step for x, 2-byte stores for y.  Statistics are taken from the fp32 value.
template <int PLANES, bool TR, bool STATS, bool RES, bool XB = false, bool YB = false>
__global__ __launch_bounds__(512, 1) void conv1x1_bf16_il_kernel(BfArgs a) {
  static_assert(!(XB || YB) || PLANES == 1, "bf16 rows go with bf16 products");
  constexpr int XE = XB ? 2 : 4;  // bytes per activation element of x
  using L = IlLds<PLANES>;
  using AR = Arith<PLANES>;
  using x8 = typename AR::x8;
  using x2 = typename AR::x2;
  constexpr int D = L::D, NA = L::NA;
  // Counted wait at the end of interval g: A(g+1) and x(g+3) have landed.  Per interval a wave issues its PLANES weight
  // pieces (of A(g + NA - 1)) and then its PX activation pieces (of x(g + D + 1)); vmcnt retires in issue order, so the
  // wait may leave outstanding whatever was issued after the younger of the two.
  constexpr int PX = XB ? 1 : 2, PER = PLANES + PX;
  constexpr int VM_A = PX + (NA - 2) * PER, VM_X = (D - 2) * PER;
  constexpr int VMW = VM_A < VM_X ? VM_A : VM_X;
  __shared__ __attribute__((aligned(16))) unsigned char smem[L::TOTAL];
  float* tab = reinterpret_cast<float*>(smem + L::OFF_TAB);
  float* bias_lds = reinterpret_cast<float*>(smem + L::OFF_BIAS);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = wave >> 2;  // half
  const int hw = wave & 3;
  const int ptid = tid & 255;
  const int wm = hw >> 1, wt = hw & 1;
  const int lr = lane & 31, lh = lane >> 5;

  const int S = a.ksteps;
  const int st_per = (a.tiles_t + 1) >> 1;
  const int nsuper = st_per * a.tiles_m * a.N;
  const int G = gridDim.x;
  int vb = blockIdx.x;  // position in the supertile order
  if (a.pair_r > 0) {   // (utterance, m-tile, part of the row) with the m-tile taken from bit 3 of blockIdx
    const int xcd = vb & 7, j = vb >> 3;
    const int u = (j >> 1) * 8 + xcd;
    vb = ((u / a.pair_r) * 2 + (j & 1)) * a.pair_r + u % a.pair_r;
  }
  const int lo = (int)((long long)vb * nsuper / G), hi = (int)((long long)(vb + 1) * nsuper / G);
  if (lo >= hi) return;
  const int total = (hi - lo) * S;
  // supertile index -> utterance, m-tile, pair of t-tiles.  (out_conv, two m-tiles, reads its input tile once per
  // m-tile: PMC FETCH_SIZE 550 MB against 415 MB algorithmic at 32 utterances.  Running the m-tile fastest instead does
  // not bring the second read out of L2 -- 32 workgroups x 256 KiB per XCD exceed its 4 MiB -- and changed nothing.)
  auto decode = [&](int idx, int& n, int& mt, int& t2) {
    t2 = idx % st_per;
    const int r = idx / st_per;
    mt = r % a.tiles_m;
    n = r / a.tiles_m;
  };
  int n_lo, mt_lo, t2_lo;
  decode(lo, n_lo, mt_lo, t2_lo);

  const float slope = (TR && a.pro.prelu) ? a.pro.slope[0] : 1.f;
  const int n_hi = ((hi - 1) / st_per) / a.tiles_m;
  [[maybe_unused]] float xs_u[PP_MAXU] = {1.f, 1.f}, os_u[PP_MAXU] = {1.f, 1.f};  // PLANES = 2: per-utterance scale pairs
  if constexpr (PLANES == 2) {
    f16_scales(a, n_lo, lane, xs_u[0], os_u[0]);
    xs_u[1] = xs_u[0], os_u[1] = os_u[0];
    if (n_hi > n_lo) f16_scales(a, n_lo + 1, lane, xs_u[1], os_u[1]);
  }
  // (scale / shift + PReLU prologues only: the launcher keeps the others on the ping-pong kernel)
  if constexpr (TR) {
    const bool has_norm = a.pro.norm != PS_NORM_NONE;
    for (int u = 0; u <= n_hi - n_lo; ++u) {  // every wave reduces the producer's partial statistics itself
      float mean = 0.f, rstd = 1.f;
      if (a.pro.norm == PS_NORM_GLOBAL) {
        double sa = 0.0, sq = 0.0;
        const double* src = a.pro.stats + (size_t)(n_lo + u) * a.pro.parts * 2;
        for (int i = lane; i < a.pro.parts; i += 64) {
          sa += src[2 * i];
          sq += src[2 * i + 1];
        }
        sa = wave_sum(sa);
        sq = wave_sum(sq);
        const double m = sa / a.pro.count;
        double var = sq / a.pro.count - m * m;
        var = var < 0.0 ? 0.0 : var;  // (a NaN variance -- the utterance holds an infinity -- stays NaN, as in torch)
        mean = (float)m;
        rstd = (float)(1.0 / sqrt(var + (double)a.pro.eps));
      }
      const int k = tid;  // 512 threads, 512 table rows
      float sc = 0.f, sh = 0.f;
      if (k < a.K) {
        sc = has_norm ? a.pro.gamma[k] * rstd : 1.f;
        sh = has_norm ? a.pro.beta[k] - mean * sc : 0.f;
      }
      if constexpr (PLANES == 2) sc *= xs_u[u & 1], sh *= xs_u[u & 1];  // (PReLU commutes with a positive scale)
      tab[u * 1024 + k] = sc;
      tab[u * 1024 + 512 + k] = sh;
    }
  }

  // ---- activation DMA: raw fp32 [16][128] of one K-step -> ring slot --------------------------------------------------
  // fp32 rows: a piece (64 lanes x 16 B) covers two rows of 128 frames, a wave issues two pieces (rows 2 hw, 2 hw + 1
  // and the same + 8); bf16 rows: a piece covers four rows, a wave issues one (rows 4 hw .. 4 hw + 3)
  const int x_voff = XB ? ((lane >> 4) * a.ldt + (lane & 15) * 8) * 2 : ((lane >> 5) * a.ldt + (lane & 31) * 4) * 4;
  const int x_step = XB_K * a.ldt * XE, x_half = 8 * a.ldt * XE;
  float* const raw_w = reinterpret_cast<float*>(smem + L::OFF_RAW + h * D * L::RAW) + hw * 256;
  int xi = lo, xk = 0, xso = 0;  // supertile, step, scalar offset of the step's first row of this wave
  __amdgpu_buffer_rsrc_t xr;
  auto x_setup = [&]() {
    int n, mt, t2;
    decode(xi, n, mt, t2);
    bool ok = xi < hi && 2 * t2 + h < a.tiles_t;  // past the end / tile outside the row: empty descriptor
#ifdef PS_PP_STAMPS
    if (a.ablate & 2) ok = false;  // timing experiment: the DMA instructions stay, their traffic goes
#endif
    xr = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<unsigned char*>(const_cast<float*>(a.x)) + (size_t)n * a.K * a.ldt * XE, 0,
        ok ? a.K * a.ldt * XE : 0, 0x00020000);
    xso = (hw * (XB ? 4 : 2) * a.ldt + (2 * t2 + h) * XB_T) * XE;
  };
  auto dma_x = [&](int slot) {
    float* dst = raw_w + slot * (L::RAW / 4);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, dst, 16, x_voff, xso, 0, IL_X_AUX);
    if constexpr (!XB) __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, dst + 1024, 16, x_voff, xso + x_half, 0, IL_X_AUX);
  };
  auto dma_x1 = [&](int slot, auto half_c) {  // one of the two pieces
    constexpr int hf = decltype(half_c)::value;
    float* dst = raw_w + slot * (L::RAW / 4);
    if constexpr (!XB || hf == 0)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, dst + hf * 1024, 16, x_voff, xso + hf * x_half, 0, IL_X_AUX);
  };
  auto x_advance = [&]() {
    xso += x_step;
    if (++xk == S) {
      xk = 0;
      ++xi;
      x_setup();
    }
  };

  // ---- weight DMA: this half's share (half a slot) of one K-step, already in its LDS image ----------------------------
  const int w_voff = lane * 16;
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.wt), 0, a.tiles_m * S * L::A_SLOT, 0x00020000);
  // A wave fetches the 32-row block (all planes) its own MFMAs start a step with: row block (rot + p) & 3 of its 128 rows
  // is the p-th it works on, rot = 2 h + wt numbers the four waves that share those rows.  So the fragments of a step's
  // first row block can be read as soon as the wave's own pieces have landed -- before the barrier that publishes the
  // rest of the slot -- and no MFMA waits for a fragment read after the barrier.
  const int rot = h * 2 + wt;
  const int a_share = (wm * 4 + rot) * 1024;  // byte offset of this wave's piece of plane 0 inside a slot
  int ai = lo, ak = 0, aso = 0;
  auto a_setup = [&]() {
    int n, mt, t2;
    decode(ai, n, mt, t2);
    aso = ai < hi ? mt * S * L::A_SLOT + a_share : 0x7f000000;  // past the end: outside the descriptor
#ifdef PS_PP_STAMPS
    if (a.ablate & 2) aso = 0x7f000000;
#endif
  };
  auto dma_a = [&](int slot) {
    float* dst = reinterpret_cast<float*>(smem + slot * L::A_SLOT + a_share);
#pragma unroll
    for (int i = 0; i < PLANES; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, dst + i * 2048, 16, w_voff, aso + i * 8192, 0, 0);
  };
  auto dma_a1 = [&](int slot, auto i_c) {  // one of the PLANES pieces
    constexpr int i = decltype(i_c)::value;
    float* dst = reinterpret_cast<float*>(smem + slot * L::A_SLOT + a_share);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, dst + i * 2048, 16, w_voff, aso + i * 8192, 0, 0);
  };
  auto a_advance = [&]() {
    aso += L::A_SLOT;
    if (++ak == S) {
      ak = 0;
      ++ai;
      a_setup();
    }
  };

  auto bias_dma = [&](int n, int mt, int par) {
    const __amdgpu_buffer_rsrc_t br = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.bias ? a.bias : a.x), 0, a.bias ? a.M * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t bnr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.bias_n ? a.bias_n + (size_t)n * a.M : a.x), 0, a.bias_n ? a.M * 4 : 0, 0x00020000);
    float* dst = bias_lds + par * 2 * XB_M;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(br, dst, 16, w_voff, mt * XB_M * 4, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(bnr, dst + XB_M, 16, w_voff, mt * XB_M * 4, 0, 0);
  };

  // ---- staging: raw ring slot -> one of this half's bf16 slots, in chunks (S_load, S_tr, S_split, S_write) -------------
  const int bt = ptid & 127, bh = ptid >> 7;  // frame, k-half
  const float* const raw_r = reinterpret_cast<const float*>(smem + L::OFF_RAW + h * D * L::RAW) + 8 * bh * XB_T + bt;
  unsigned char* const bx_w = smem + L::OFF_B + h * L::NB * L::B_SLOT + (bt * XB_K + 8 * bh) * 2;
  int si = lo, sk = 0, spar = 0;  // supertile, step, bias-table parity of the step to stage next
  int srs = 0, sbs = 0;           // raw ring slot / bf16 slot of the step to stage next
  const float* stab = tab + 8 * bh;
  [[maybe_unused]] float sxs = xs_u[0];  // PLANES = 2, no prologue: scale of the utterance being staged
  auto s_setup = [&]() {
    int n, mt, t2;
    decode(si, n, mt, t2);
    stab = tab + (n - n_lo) * 1024 + 8 * bh;
    if constexpr (PLANES == 2) sxs = n == n_lo ? xs_u[0] : xs_u[1];
    if (wave == 0 && si < hi) bias_dma(n, mt, spar);
  };
  float sv[8];
  f32x4 sc0, sc1, sh0, sh1;
  x8 piece[PLANES];
  auto S_load = [&]() {
    if constexpr (XB) {  // raw slot = [16 k][128 t] bf16 (the first 4 KiB of the slot)
      const unsigned short* raw = reinterpret_cast<const unsigned short*>(smem + L::OFF_RAW + (h * D + srs) * L::RAW) +
                                  8 * bh * XB_T + bt;
#pragma unroll
      for (int j = 0; j < 8; ++j) sv[j] = __builtin_bit_cast(float, (unsigned)raw[j * XB_T] << 16);
    } else {
      const float* raw = raw_r + srs * (L::RAW / 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) sv[j] = raw[j * XB_T];
    }
    if constexpr (TR) {
      sc0 = *reinterpret_cast<const f32x4*>(stab), sc1 = *reinterpret_cast<const f32x4*>(stab + 4);
      sh0 = *reinterpret_cast<const f32x4*>(stab + 512), sh1 = *reinterpret_cast<const f32x4*>(stab + 516);
    }
  };
  auto S_tr = [&](auto lo_c) {  // prologue transform of four values (scale / shift + PReLU; the launcher routes the
    constexpr int j0 = decltype(lo_c)::value;  // ReLU-before / tanh-after prologues to the ping-pong kernel)
    if constexpr (TR) {
#pragma unroll
      for (int j = j0; j < j0 + 4; ++j)
        sv[j] = prelu(sv[j] * (j < 4 ? sc0[j & 3] : sc1[j & 3]) + (j < 4 ? sh0[j & 3] : sh1[j & 3]), slope);
    } else if constexpr (PLANES == 2) {
#pragma unroll
      for (int j = j0; j < j0 + 4; ++j) sv[j] *= sxs;
    }
  };
  auto S_split = [&](auto p_c, auto j_c) {  // plane p of the pairs (j0, j0+1), (j0+2, j0+3)
    constexpr int p = decltype(p_c)::value, j0 = decltype(j_c)::value;
#pragma unroll
    for (int j = j0; j < j0 + 4; j += 2) {
      const x2 hh = __builtin_convertvector(f32x2v{sv[j], sv[j + 1]}, x2);
      piece[p][j] = hh[0];
      piece[p][j + 1] = hh[1];
      if constexpr (p + 1 < PLANES) {
        const f32x2v back = __builtin_convertvector(hh, f32x2v);
        sv[j] -= back[0];
        sv[j + 1] -= back[1];
      }
    }
  };
  auto S_write = [&](auto p_c) {
    constexpr int p = decltype(p_c)::value;
    *reinterpret_cast<x8*>(bx_w + sbs * L::B_SLOT + p * XB_T * XB_K * 2) = piece[p];
  };
  auto stage_all = [&]() {  // the whole staging of one step in one go (prologue)
    S_load();
    S_tr(bic<0>{});
    S_tr(bic<4>{});
    if constexpr (PLANES == 3) {
      S_split(bic<0>{}, bic<0>{}), S_split(bic<0>{}, bic<4>{}), S_write(bic<0>{});
      S_split(bic<1>{}, bic<0>{}), S_split(bic<1>{}, bic<4>{}), S_write(bic<1>{});
      S_split(bic<2>{}, bic<0>{}), S_split(bic<2>{}, bic<4>{}), S_write(bic<2>{});
    } else if constexpr (PLANES == 2) {
      S_split(bic<0>{}, bic<0>{}), S_split(bic<0>{}, bic<4>{}), S_write(bic<0>{});
      S_split(bic<1>{}, bic<0>{}), S_split(bic<1>{}, bic<4>{}), S_write(bic<1>{});
    } else {
      S_split(bic<0>{}, bic<0>{}), S_split(bic<0>{}, bic<4>{}), S_write(bic<0>{});
    }
  };
  auto s_advance = [&]() {
    stab += XB_K;
    srs = srs + 1 == D ? 0 : srs + 1;
    sbs ^= 1;
    if (++sk == S) {
      sk = 0;
      ++si;
      spar ^= 1;
      s_setup();
    }
  };

  // ---- compute side ---------------------------------------------------------------------------------------------------
  f32x16 acc[4][2];
  const int lane_off = (4 * lh * a.ldt + lr) * 4;
  auto tile_ok = [&](int idx, int t2) { return idx < hi && 2 * t2 + h < a.tiles_t; };
  auto init_acc = [&](int idx) {
    if constexpr (RES) {
      int n, mt, t2;
      decode(idx, n, mt, t2);
      constexpr int RE = YB ? 2 : 4;
      const int slab = a.M * a.ldt * RE;
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
          reinterpret_cast<unsigned char*>(const_cast<float*>(a.res)) + (size_t)n * a.M * a.ldt * RE, 0,
          tile_ok(idx, t2) ? slab : 0, 0x00020000);
      const int tile_off = ((mt * XB_M + wm * 128) * a.ldt + (2 * t2 + h) * XB_T + wt * 64) * 4;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rc = ((rot + mi) & 3) * 32 + (r & 3) + 8 * (r >> 2);
#pragma unroll
          for (int ti = 0; ti < 2; ++ti) {
            if constexpr (YB)  // (bf16 output rows: the residual stream is bf16 as well)
              acc[mi][ti][r] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(
                                                             rr, lane_off >> 1, (tile_off + rc * a.ldt * 4 + ti * 128) >> 1, IL_RS_AUX) << 16);
            else
              acc[mi][ti][r] = __builtin_bit_cast(
                  float, __builtin_amdgcn_raw_buffer_load_b32(rr, lane_off, tile_off + rc * a.ldt * 4 + ti * 128, IL_RS_AUX));
          }
        }
    } else {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mi][ti][r] = 0.f;
    }
  };
  // PLANES = 2 with a residual: the accumulators count in scaled units (2^(w_exp + x_exp)), so the residual they start
  // from is brought there too (a power of two: exact) once its loads have landed
  auto scale_res = [&](int idx) {
    if constexpr (PLANES == 2 && RES) {
      int n, mt, t2;
      decode(idx, n, mt, t2);
      const float inv = 1.f / (n == n_lo ? os_u[0] : os_u[1]);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mi][ti][r] *= inv;
    }
  };
  auto acc_fence = [&]() {
    asm volatile("" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[2][0]),
                 "+v"(acc[2][1]), "+v"(acc[3][0]), "+v"(acc[3][1]));
  };

  const unsigned char* a_frag[4];  // row block the wave works on p-th
#pragma unroll
  for (int p4 = 0; p4 < 4; ++p4) a_frag[p4] = smem + ((wm * 128 + ((rot + p4) & 3) * 32 + lr) * XB_K + 8 * lh) * 2;
  const unsigned char* const b_frag = smem + L::OFF_B + h * L::NB * L::B_SLOT + ((wt * 64 + lr) * XB_K + 8 * lh) * 2;
  x8 bf[PLANES][2];  // B fragments of the step the next MFMAs consume (loaded before the barrier)
  auto read_bplane = [&](int bslot, auto p_c) {
    constexpr int p = decltype(p_c)::value;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
      bf[p][ti] = *reinterpret_cast<const x8*>(b_frag + bslot * L::B_SLOT + (p * XB_T + ti * 32) * XB_K * 2);
  };
  auto read_bfrags = [&](int bslot) {
    read_bplane(bslot, bic<0>{});
    if constexpr (PLANES >= 2) read_bplane(bslot, bic<1>{});
    if constexpr (PLANES == 3) read_bplane(bslot, bic<2>{});
  };
  x8 af[2][PLANES];
  auto read_afrags = [&](int sa, auto mi_c) {  // sa: byte offset of the weight slot
    constexpr int mi = decltype(mi_c)::value;
    constexpr int ORD_A[3] = {1, 2, 0};  // in the order the MFMAs use them
#pragma unroll
    for (int q = 0; q < PLANES; ++q) {
      const int pa = PLANES == 3 ? ORD_A[q] : PLANES == 2 ? 1 - q : 0;
      af[mi & 1][pa] = *reinterpret_cast<const x8*>(a_frag[mi] + sa + pa * XB_M * XB_K * 2);
    }
  };
  // group q of row block mi: PLANES = 3: two of the six products (smallest terms first: (W1,x1) (W2,x0) | (W0,x2) (W1,x0) |
  // (W0,x1) (W0,x0)) on both column blocks = 4 MFMAs; PLANES = 1: the one product on both column blocks
  auto mf_group = [&](auto mi_c, auto q_c) {
    constexpr int mi = decltype(mi_c)::value, q = decltype(q_c)::value;
    constexpr int PA[6] = {1, 2, 0, 1, 0, 0}, PB[6] = {1, 0, 2, 0, 1, 0};
    const x8* f = af[mi & 1];
    if constexpr (PLANES == 3) {
#pragma unroll
      for (int e = 2 * q; e < 2 * q + 2; ++e)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) acc[mi][ti] = AR::mfma(f[PA[e]], bf[PB[e]][ti], acc[mi][ti]);
    } else if constexpr (PLANES == 2) {  // group q = one product on both column blocks: (W1,x0) | (W0,x1) | (W0,x0)
      constexpr int PA2[3] = {1, 0, 0}, PB2[3] = {0, 1, 0};
      if constexpr (IL_F16_NQ == 3) {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) acc[mi][ti] = AR::mfma(f[PA2[q]], bf[PB2[q]][ti], acc[mi][ti]);
      } else {  // one group per row block: all three products
#pragma unroll
        for (int e = 0; e < 3; ++e)
#pragma unroll
          for (int ti = 0; ti < 2; ++ti) acc[mi][ti] = AR::mfma(f[PA2[e]], bf[PB2[e]][ti], acc[mi][ti]);
      }
    } else {
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) acc[mi][ti] = AR::mfma(f[0], bf[0][ti], acc[mi][ti]);
    }
  };

  // (An LDS-transposed drain -- four registers per round through the wave's own pieces of the released weight slot,
  //  read back row-major and stored as dwordx4 over whole cache lines, 32 stores per tile and wave instead of 128 -- was
  //  built and measured: 10-15 k cycles per tile against 10-15 k with statistics, 38 k against 22-37 k with the residual.
  //  With every CU draining at the same step the drain runs at the chip's write (+ residual read) bandwidth, not at the
  //  store-issue rate: 256 KiB per CU and supertile.  The direct form stays.)
  // finished tile of supertile idx: bias, statistics, stores; then the accumulators take the residual of this half's
  // next tile.  Element (mi, ti, r) = row 128 wm + 32 ((rot + mi) & 3) + (r&3) + 8 (r>>2) + 4 lh, column 64 wt + 32 ti + lr.
  auto drain = [&](int idx, int parity) {
    int n, mt, t2, nn, nmt, nt2;
    decode(idx, n, mt, t2);
    decode(idx + 1, nn, nmt, nt2);
    const bool ok = 2 * t2 + h < a.tiles_t;
    const int m0 = mt * XB_M, t0 = (2 * t2 + h) * XB_T;
    float fsum = 0.f, fsq = 0.f;
    [[maybe_unused]] float amx2[2] = {0.f, 0.f};  // per column block; the pad-frame mask is applied once at the end
    [[maybe_unused]] const float osc = n == n_lo ? os_u[0] : os_u[1];
    constexpr int YE = YB ? 2 : 4;
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<unsigned char*>(a.y) + (size_t)n * a.M * a.ldt * YE, 0, ok ? a.M * a.ldt * YE : 0, 0x00020000);
    const int tile_off = ((m0 + wm * 128) * a.ldt + t0 + wt * 64) * 4;
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<unsigned char*>(const_cast<float*>(RES ? a.res : a.y)) + (size_t)nn * a.M * a.ldt * YE, 0,
        (RES && tile_ok(idx + 1, nt2)) ? a.M * a.ldt * YE : 0, 0x00020000);
    [[maybe_unused]] const int ntile_off = ((nmt * XB_M + wm * 128) * a.ldt + (2 * nt2 + h) * XB_T + wt * 64) * 4;
    bool cm[2];  // (a select, not a 0/1 factor: 0 * NaN would poison the statistics)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) cm[ti] = t0 + wt * 64 + ti * 32 + lr < a.T;
    const float* bl = bias_lds + parity * 2 * XB_M + wm * 128 + 4 * lh;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int pb = ((rot + mi) & 3) * 32;  // first row of the block
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(bl + pb + 8 * rq) +
                         *reinterpret_cast<const f32x4*>(bl + XB_M + pb + 8 * rq);
#pragma unroll
        for (int r3 = 0; r3 < 4; ++r3) {
          const int r = rq * 4 + r3;
          const int rc = pb + r3 + 8 * rq;
#pragma unroll
          for (int ti = 0; ti < 2; ++ti) {
            const float v = PLANES == 2 ? acc[mi][ti][r] * osc + b4[r3] : acc[mi][ti][r] + b4[r3];
            // (as an instruction of its own: left to hipcc, the 256 maxima of the residual variant become a
            //  reduction tree that keeps every value alive and spills 53 registers -- 87 MB of scratch per launch)
            if constexpr (PLANES == 2) asm volatile("v_max_f32 %0, %0, |%1|" : "+v"(amx2[ti]) : "v"(v));
            if constexpr (STATS) {
              const float vm = cm[ti] ? v : 0.f;
              fsum += vm;
              fsq += vm * vm;
            }
            if constexpr (YB)
              __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (__bf16)v), yr, lane_off >> 1,
                                                    (tile_off + rc * a.ldt * 4 + ti * 128) >> 1, 0);
            else
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yr, lane_off,
                                                    tile_off + rc * a.ldt * 4 + ti * 128, IL_ST_AUX);
            if constexpr (RES && YB)
              acc[mi][ti][r] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(
                                                             rr, lane_off >> 1, (ntile_off + rc * a.ldt * 4 + ti * 128) >> 1, IL_RS_AUX) << 16);
            else if constexpr (RES)
              acc[mi][ti][r] = __builtin_bit_cast(
                  float, __builtin_amdgcn_raw_buffer_load_b32(rr, lane_off, ntile_off + rc * a.ldt * 4 + ti * 128, IL_RS_AUX));
            else
              acc[mi][ti][r] = 0.f;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if constexpr (STATS) {
      const double s = wave_sum_dpp(fsum), q = wave_sum_dpp(fsq);
      if (lane == 0 && ok) {
        const int parts = a.tiles_m * a.tiles_t * 4;
        const int part = (mt * a.tiles_t + 2 * t2 + h) * 4 + hw;
        double* dst = a.ostats + ((size_t)n * parts + part) * 2;
        dst[0] = s;
        dst[1] = q;
      }
    }
    if constexpr (PLANES == 2) {
      if (a.y_amax) {
        const float amx = wave_max(fmaxf(cm[0] ? amx2[0] : 0.f, cm[1] ? amx2[1] : 0.f));
        if (lane == 0 && ok)
          a.y_amax[(size_t)n * (a.tiles_m * a.tiles_t * 4) + (mt * a.tiles_t + 2 * t2 + h) * 4 + hw] = amx;
      }
    }
  };

  // ---- prologue ----------------------------------------------------------------------------------------------------------
  if (a.delay > 0) {  // start offset between phases of workgroups (see bf16_launch); every XCD holds all phases
    const int grp = (a.pair_r > 0 ? blockIdx.x >> 4 : blockIdx.x >> 3) % a.groups;  // (paired workgroups share a phase)
    unsigned long long t_start, now;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_start)::"memory");
    const unsigned long long until = t_start + (unsigned long long)grp * a.delay;
    do {
      __builtin_amdgcn_s_sleep(32);
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
    } while (now < until);
  }
  x_setup();
  a_setup();
#pragma unroll
  for (int j = 0; j < D; ++j) {  // x(0..2) -> raw slots 0..2
    dma_x(j);
    x_advance();
  }
#pragma unroll
  for (int j = 0; j < NA - 1; ++j) {  // A(0 .. NA-2) -> weight slots 0 .. NA-2
    dma_a(j);
    a_advance();
  }
  if (wave == 0) bias_dma(n_lo, mt_lo, 0);
  init_acc(lo);
  acc_fence();
  scale_res(lo);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // tables, raw steps 0..2 and weight slot 0 are in LDS
  // steps 0 and 1 -> bf16 slots 0 and 1 (S >= 4: both belong to the first supertile, whose bias rows are in flight)
  stage_all();
  stab += XB_K, srs = 1, sbs = 1, sk = 1;
  stage_all();
  stab += XB_K, srs = 2, sbs = 0, sk = 2;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  read_bfrags(0);
  dma_x(0);  // x(D) -> raw slot 0 (the "interval -1" issue)
  x_advance();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // every wave holds its fragments of step 0: bf16 slot 0 may be rewritten
  asm volatile("" ::: "memory");
  int rx = 1;               // raw ring slot the x DMA of this interval goes to ((g + D + 1) % D)
  int wa = (NA - 1) % NA;   // weight slot the A DMA of this interval goes to ((g + NA - 1) % NA)

#ifdef PS_PP_STAMPS
  unsigned long long il_m = 0, il_w = 0, il_d = 0, il_t0 = 0, il_prev = 0, il_rt0 = 0;
  if (a.stamps) {
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(il_rt0)::"memory");  // constant 100 MHz
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(il_t0)::"memory");
    il_prev = il_t0;
  }
#define IL_STAMP(bucket)                                                          \
  if (a.stamps) {                                                                 \
    unsigned long long now;                                                       \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory"); \
    bucket += now - il_prev;                                                      \
    il_prev = now;                                                                \
  }
#else
#define IL_STAMP(bucket)
#endif

  // ---- main loop: interval g = MFMAs of step g with the chunks of [DMA A(g+1), x(g+4)] and [staging of step g+2] between
  // them; B fragments of step g+1; counted wait (everything but x(g+4)); barrier; a finished tile's drain -------------------
  // chunk `idx` of the interval's side work (PLANES = 3: 12 slots, one per group of four MFMAs; PLANES = 1: 4 slots).
  // One DMA instruction per slot: the next piece's M0 write waits for the piece before it, and three pieces back to
  // back stall the wave (and its MFMAs) for several hundred cycles.  (Tried, no gain: half 1 running one chunk ahead
  // of half 0; every wave issuing its DMA pieces in a slot of its own.)
  auto chunk = [&](auto idx_c) {
    constexpr int idx = decltype(idx_c)::value;
    if constexpr (PLANES == 3) {
      if constexpr (idx == 0) S_load();  // (the raw reads land while the next MFMA groups issue)
      if constexpr (idx == 0) dma_a1(wa, bic<0>{});
      if constexpr (idx == 1) dma_a1(wa, bic<1>{});
      if constexpr (idx == 2) dma_a1(wa, bic<2>{});
      if constexpr (idx == 3) dma_x1(rx, bic<0>{});
      if constexpr (idx == 4) dma_x1(rx, bic<1>{});
      if constexpr (idx == 2) S_tr(bic<0>{});
      if constexpr (idx == 3) S_tr(bic<4>{});
      if constexpr (idx == 4) S_split(bic<0>{}, bic<0>{});
      if constexpr (idx == 5) S_split(bic<0>{}, bic<4>{}), S_write(bic<0>{});
      if constexpr (idx == 6) S_split(bic<1>{}, bic<0>{});
      if constexpr (idx == 7) S_split(bic<1>{}, bic<4>{}), S_write(bic<1>{});
      if constexpr (idx == 8) S_split(bic<2>{}, bic<0>{});
      if constexpr (idx == 9) S_split(bic<2>{}, bic<4>{}), S_write(bic<2>{});
    } else if constexpr (PLANES == 2 && IL_F16_NQ == 1) {  // 4 slots, one per row block of six MFMAs
      if constexpr (idx == 0) S_load(), dma_a1(wa, bic<0>{});
      if constexpr (idx == 1) dma_a1(wa, bic<1>{}), S_tr(bic<0>{}), S_tr(bic<4>{});
      if constexpr (idx == 2) dma_x1(rx, bic<0>{}), S_split(bic<0>{}, bic<0>{}), S_split(bic<0>{}, bic<4>{}), S_write(bic<0>{});
      if constexpr (idx == 3) dma_x1(rx, bic<1>{}), S_split(bic<1>{}, bic<0>{}), S_split(bic<1>{}, bic<4>{}), S_write(bic<1>{});
    } else if constexpr (PLANES == 2) {  // 12 slots, one per pair of MFMAs
      if constexpr (idx == 0) S_load();
      if constexpr (idx == 0) dma_a1(wa, bic<0>{});
      if constexpr (idx == 1) dma_a1(wa, bic<1>{});
      if constexpr (idx == 2) S_tr(bic<0>{});
      if constexpr (idx == 3) dma_x1(rx, bic<0>{});
      if constexpr (idx == 4) S_tr(bic<4>{});
      if constexpr (idx == 5) dma_x1(rx, bic<1>{});
      if constexpr (idx == 6) S_split(bic<0>{}, bic<0>{});
      if constexpr (idx == 7) S_split(bic<0>{}, bic<4>{}), S_write(bic<0>{});
      if constexpr (idx == 8) S_split(bic<1>{}, bic<0>{});
      if constexpr (idx == 9) S_split(bic<1>{}, bic<4>{}), S_write(bic<1>{});
    } else {
      if constexpr (idx == 0) S_load(), dma_a1(wa, bic<0>{});
      if constexpr (idx == 1) dma_x1(rx, bic<0>{}), S_tr(bic<0>{}), S_tr(bic<4>{});
      if constexpr (idx == 2) dma_x1(rx, bic<1>{}), S_split(bic<0>{}, bic<0>{}), S_split(bic<0>{}, bic<4>{}), S_write(bic<0>{});
    }
  };
  constexpr int NQ = PLANES == 3 ? 3 : PLANES == 2 ? IL_F16_NQ : 1;  // MFMA groups per row block
  if (IL_PRIO1 && h == 1) __builtin_amdgcn_s_setprio(IL_PRIO1);
  int ci = lo, ck = 0;  // compute: supertile, step
  int parity = 0;       // bias-table parity of ci
  int ra = 0;           // g % NA: weight slot of step g
  read_afrags(0, bic<0>{});  // step 0 (weight slot 0 is complete)
  for (int g = 0; g < total; ++g) {
    const int sa = ra * L::A_SLOT;
    auto slot = [&](auto mi_c, auto q_c) {
      constexpr int mi = decltype(mi_c)::value, q = decltype(q_c)::value;
      if constexpr (q == 0 && mi < 3) read_afrags(sa, bic<mi + 1>{});  // requested before this row block's MFMAs issue
      __builtin_amdgcn_sched_barrier(0);
#ifdef PS_PP_STAMPS  // (diagnostic build: ps_debug_ablate 1 / 4 removes the MFMAs / the chunks)
      const bool do_chunk = !(a.ablate & 4);
      if (!(a.ablate & 1))
#else
      constexpr bool do_chunk = true;
#endif
        mf_group(mi_c, q_c);
      __builtin_amdgcn_sched_barrier(0);
      if (do_chunk) chunk(bic<mi * NQ + q>{});
      __builtin_amdgcn_sched_barrier(0);
    };
    slot(bic<0>{}, bic<0>{});
    if constexpr (NQ == 3) slot(bic<0>{}, bic<1>{}), slot(bic<0>{}, bic<2>{});
    slot(bic<1>{}, bic<0>{});
    if constexpr (NQ == 3) slot(bic<1>{}, bic<1>{}), slot(bic<1>{}, bic<2>{});
    slot(bic<2>{}, bic<0>{});
    if constexpr (NQ == 3) slot(bic<2>{}, bic<1>{}), slot(bic<2>{}, bic<2>{});
    // the B fragments of step g+1 replace those of step g plane by plane, each right behind its last MFMA of the
    // step ((W0,x2) is the third product, (W0,x1) the fifth, (W0,x0) the last), so only the x0 plane's two reads are
    // issued after the last MFMA
    const int nb = (g + 1) & 1;
    // the wave's own pieces of A(g+1) have landed (everything but x(g+4) has): first row block of the next step
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMW) : "memory");
    const int ra_next = ra + 1 == NA ? 0 : ra + 1;
    read_afrags(ra_next * L::A_SLOT, bic<0>{});
    slot(bic<3>{}, bic<0>{});
    if constexpr (PLANES == 3) {
      slot(bic<3>{}, bic<1>{});
      read_bplane(nb, bic<2>{});
      slot(bic<3>{}, bic<2>{});
      read_bplane(nb, bic<1>{});
    } else if constexpr (PLANES == 2 && NQ == 3) {
      slot(bic<3>{}, bic<1>{});
      read_bplane(nb, bic<1>{});
      slot(bic<3>{}, bic<2>{});
    } else if constexpr (PLANES == 2) {
      read_bplane(nb, bic<1>{});
    }
    read_bplane(nb, bic<0>{});
    a_advance();
    x_advance();
    s_advance();
    rx = rx + 1 == D ? 0 : rx + 1;
    wa = wa + 1 == NA ? 0 : wa + 1;
    ra = ra_next;
    IL_STAMP(il_m)
    // this wave's share of A(g+1) and its pieces of x(g+3) have landed
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(VMW) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    IL_STAMP(il_w)
    if (ck == S - 1) {
      drain(ci, parity);
      parity ^= 1;
      acc_fence();  // the wait for the residual loads belongs here, not in front of every iteration's MFMAs
      if (ci + 1 < hi) scale_res(ci + 1);
      IL_STAMP(il_d)
    }
    if (++ck == S) {
      ck = 0;
      ++ci;
    }
  }
#ifdef PS_PP_STAMPS
  if (a.stamps && (tid & 255) == 0) {
    unsigned long long now, rnow;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rnow)::"memory");
    unsigned long long* d = a.stamps + ((size_t)blockIdx.x * 2 + h) * 6;
    d[0] = now - il_t0;
    d[1] = il_m;
    d[2] = rnow - il_rt0;  // 10 ns units: d[0] / d[2] / 10 = the clock the kernel ran at, in GHz
    d[3] = il_w;
    d[4] = il_d;
    d[5] = (unsigned long long)total;
  }
#endif
}
