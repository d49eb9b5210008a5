// ---- "rb": the fp16x2 GEMM whose activations never touch LDS (included by conv1x1_bf16.hip) ---------------------------
// What rounds 2-4 measured on the three designs of this GEMM (interleaved, one-wave-per-SIMD, and a first form of this
// file on the 32x32x16 MFMA): cycles per K-step 3185 / ~2200 / 2155, in-kernel clock 1.41 / 1.25 / 1.17 GHz, wall time
// equal within 3 %.  The chip hands back in clock what a schedule saves in cycles, and the ablations say what it is
// paying for: the MFMAs with their fragment reads alone (no HBM traffic, no staging) hold the chip at 1.48 GHz and take
// 112 of the launch's 142 us; the same kernel on all-zero operands runs at 1.88 GHz.  The lever is therefore the energy
// of a multiply-add, and the one piece of it a kernel chooses is the MFMA shape: tools/probe/mfma_shape_probe.hip runs
// this kernel's MFMA skeleton (256 x 32 per wave, three products, random fp16 operands) on both shapes -- the same cycles,
// 1.54 GHz on v_mfma_f32_32x32x16_f16, 1.80-1.84 GHz on v_mfma_f32_16x16x32_f16: 10 % (fragments from LDS) to 20 %
// (operands in registers) less wall time.  Hence 16x16x32 and a K-step of 32.
//
// A wave owns ALL 256 rows of the supertile and 32 of its 256 frames.  The B fragment of v_mfma_f32_16x16x32_f16 --
// lane (c, q) holds k = 8 q .. 8 q + 7 of column c -- is "8 consecutive input channels of one frame": nobody else needs
// it, so it is produced where it is consumed:
//   * activations: column c of column block cb stands for frame 2 c + cb, so ONE buffer_load_dwordx2 per channel
//     fetches a lane's values for both column blocks (a wave instruction = four rows x 128 bytes, whole cache lines);
//     8 loads per K-step and lane, two K-steps of raw registers behind the step in use, transformed (scale / shift +
//     PReLU) and split into the two fp16 terms one step ahead of the MFMAs that use them.  No LDS traffic, no DMA, no barrier;
//   * the epilogue inherits the mapping: a lane holds frames 2 c and 2 c + 1 of a row, so tiles leave (and residuals
//     arrive) as 8-byte accesses, 64 per wave and tile instead of 128;
//   * weights: the only LDS operand.  Two slots of 32 KiB in the image [plane][k-quarter][256 rows][8 k]: the 16 lanes
//     that a ds_read_b128 serves in one cycle read 256 consecutive bytes (no bank conflicts; the [row][16 k] image of the
//     other kernels costs 43 % of its LDS cycles in conflicts).  The image is made by the DMA itself: lane i of a piece
//     fetches the 16 bytes (row i, 8 k) of the packer's [plane][row][16 k] slots (per-lane source offset i * 32);
//   * per K-step (32) and wave: 32 A-fragment reads (two per row block, requested one row block ahead), 96 MFMAs,
//     8 DMA issues, 8 loads, ~110 vector instructions of transform cut into chunks behind the row blocks' MFMAs; ONE
//     workgroup barrier (it publishes the other weight slot).
// The loads are inline asm: next to LDS-DMA hipcc waits vmcnt(0) at the first use of an ordinary load's result, which
// would drain the pipeline every step.  Their completion is counted by hand (vmcnt retires in issue order): interval g
// issues [8 weight pieces of A(g + 1)] early and [8 loads of x(g + 3)] late, and then needs A(g + 1) and x(g + 2).
//
// TWO workgroups of four waves per CU, each with its own 256 x 128 tile and weight ring.  One workgroup of eight waves
// (the first form of this kernel) ran the K loop and the drain of its tile strictly one after the other -- vmcnt also
// counts stores, in order, so the first counted wait of the next K loop is a wait for the tile's stores -- and out_conv,
// whose drain moves 512 KiB per CU and tile, came out at K-loop time PLUS drain time (180 us for 130 us of HBM time and
// 55 us of matrix-pipe time).  Two independent workgroups drift apart (the launcher starts the second half of the grid
// half a K loop late), so one is in its K loop while the other drains.  The price is the weight traffic from L2 (each
// workgroup fetches its own copy) and twice the LDS-DMA issues per wave.
// (A four-slot register ring transformed in place -- two K-steps in flight for the same 64 registers -- was tried: hipcc
//  does not lay the raw pairs and the fragment tuples of a slot over each other, wants ~310 registers and spills the
//  very registers the loads are still writing.  So: two raw slots + two fragment sets.)
struct RbLds {
  static constexpr int KS = 32;                        // k per step
  static constexpr int A_SLOT = 2 * 4 * XB_M * 16;     // 32 KiB: [plane][k-quarter][256 rows][8 k] fp16
  static constexpr int NA = 2;
  static constexpr int OFF_TAB = NA * A_SLOT;                    // [PP_MAXU][sc[512] | sh[512]] floats
  static constexpr int OFF_BIAS = OFF_TAB + PP_MAXU * 1024 * 4;  // [2 parities][bias[256] | bias_n[256]] floats
  static constexpr int TOTAL = OFF_BIAS + 4 * XB_M * 4;          // 76 KiB
};
static_assert(2 * RbLds::TOTAL <= 160 * 1024, "two workgroups per CU");

// R16: the rows of x, y and the residual are bf16 in HBM and every operand enters the product as ONE fp16 term (the second
// term of a bf16-stored activation is zero anyway, and the weights' first fp16 term carries 11 bits against bf16's 8):
// "bf16 storage / fp32 accumulate", the arithmetic BASELINE.json names for its config 3, at a third of the MFMAs.  A
// lane's two frames are one 32-bit word, so the loads, the stores and the residual loads are 4-byte accesses.
#ifndef PS_FM_AUX
#define PS_FM_AUX 0  // cache policy of the frame-major stores (2 = nt)
#endif
template <bool TR, bool STATS, bool RES, bool R16 = false, bool FM = false, bool LN = false>
__global__ __launch_bounds__(256, 2) void conv1x1_f16x2_rb_kernel(BfArgs a) {
  static_assert(!FM || (!STATS && !RES && !R16), "frame-major output: plain fp32 epilogue only");
  static_assert(!LN || (!STATS && !RES && !R16 && !FM), "LayerNorm epilogue: fp32 rows, no statistics, its own residual");
  using L = RbLds;
  using x8 = f16x8;
  using x2 = f16x2;
  // everything but the youngest VMW operations has completed: A(g+1) was issued early in interval g, followed by x(g+3)
  constexpr int VMW = 8;  // (R16 issues four weight pieces instead of eight: the count only has to cover the loads)
  __shared__ __attribute__((aligned(16))) unsigned char smem[L::TOTAL];
  float* tab = reinterpret_cast<float*>(smem + L::OFF_TAB);
  float* bias_lds = reinterpret_cast<float*>(smem + L::OFF_BIAS);
  const int tid = threadIdx.x, lane = tid & 63;
  const int hw = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave's 32-frame strip of the tile
  const int lc = lane & 15, lq = lane >> 4;
  const int S = a.ksteps >> 1;  // (the launcher sends even ksteps only)

  // Tile index -> (utterance n, 128-frame tile tt, m-tile mt).  One m-tile: a workgroup owns a contiguous run of frame
  // tiles.  Two m-tiles (out_conv) with pair_r > 0: workgroups b and b + 8 -- same XCD under round-robin placement,
  // dispatched together -- own the SAME run of frame tiles, one m-tile each, so the second read of an activation tile is
  // an L2 hit instead of HBM traffic (PMC: 822 MB per launch with the m-tiles back to back on one workgroup, against
  // 655 MB algorithmic).  Four m-tiles (the 1024 gate rows of a bidirectional LSTM's input projection, K = 128): the same
  // with quads.  Placement is speed only: any mapping computes the same result.
  const int G = gridDim.x;
  int vb = blockIdx.x, mt_fixed = -1, units = a.tiles_t * a.tiles_m * a.N, groups = G;
  if (a.pair_r > 0) {  // (two or four m-tiles: the partners are 8, 16, 24 workgroups on)
    const int xcd = vb & 7, j = vb >> 3;
    mt_fixed = j % a.tiles_m;
    vb = (j / a.tiles_m) * 8 + xcd;   // pair / quad index
    units = a.tiles_t * a.N;          // frame tiles
    groups = G / a.tiles_m;
  }
  const int lo = (int)((long long)vb * units / groups), hi = (int)((long long)(vb + 1) * units / groups);
  if (lo >= hi) return;
  const int total = (hi - lo) * S;
  auto decode = [&](int idx, int& n, int& mt, int& tt) __attribute__((always_inline)) {
    int r = idx;
    if (mt_fixed < 0) {
      mt = idx % a.tiles_m;
      r = idx / a.tiles_m;
    } else {
      mt = mt_fixed;
    }
    tt = r % a.tiles_t;
    n = r / a.tiles_t;
  };
  int n_lo, mt_lo, tt_lo;
  decode(lo, n_lo, mt_lo, tt_lo);
  int n_hi, mt_hi, tt_hi;
  decode(hi - 1, n_hi, mt_hi, tt_hi);

  const float slope = (TR && a.pro.prelu) ? a.pro.slope[0] : 1.f;
  float xs_u[PP_MAXU] = {1.f, 1.f}, os_u[PP_MAXU] = {1.f, 1.f};  // per-utterance scale pairs (powers of two)
  f16_scales(a, n_lo, lane, xs_u[0], os_u[0]);
  xs_u[1] = xs_u[0], os_u[1] = os_u[0];
  if (n_hi > n_lo) f16_scales(a, n_lo + 1, lane, xs_u[1], os_u[1]);
  if constexpr (TR) {  // sc = gamma * rstd * xscale, sh = (beta - mean * gamma * rstd) * xscale per utterance and channel
    const bool has_norm = a.pro.norm != PS_NORM_NONE;
    for (int u = 0; u <= n_hi - n_lo; ++u) {
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
      for (int k = tid; k < 512; k += 256) {
        float sc = 0.f, sh = 0.f;
        if (k < a.K) {
          sc = has_norm ? a.pro.gamma[k] * rstd : 1.f;
          sh = has_norm ? a.pro.beta[k] - mean * sc : 0.f;
        }
        tab[u * 1024 + k] = sc * xs_u[u & 1];  // (PReLU commutes with a positive scale)
        tab[u * 1024 + 512 + k] = sh * xs_u[u & 1];
      }
    }
  }

  // ---- activations: 8 dwordx2 loads per K-step, lane (c, q) <- x[32 step + 8 q + j][t0 + 2 c, + 1], j = 0..7 ---------------
  constexpr int ES = R16 ? 2 : 4;  // bytes per activation element in HBM
  const int row_b = a.ldt * ES;
  const int x_voff = (8 * lq * a.ldt + 2 * lc) * ES;
  const int x_step = L::KS * row_b;
  int xi = lo, xk = 0, xso = 0;
  u32x4v xr;  // raw buffer descriptor of the utterance being loaded (empty past the end / for a tile outside the row)
  auto x_setup = [&]() __attribute__((always_inline)) {
    int n, mt, tt;
    decode(xi, n, mt, tt);
    bool ok = xi < hi;
#ifdef PS_PP_STAMPS
    if (a.ablate & 2) ok = false;  // timing experiment: the loads stay, their traffic goes
#endif
    const unsigned long long base = reinterpret_cast<unsigned long long>(a.x) + (unsigned long long)n * a.K * a.ldt * (unsigned long long)ES;
    xr[0] = (unsigned)base;
    xr[1] = (unsigned)(base >> 32) & 0xffffu;
    xr[2] = ok ? (unsigned)(a.K * a.ldt * ES) : 0u;
    xr[3] = 0x00020000u;
    xso = (tt * XB_T + hw * 32) * ES;
  };
  auto x_advance = [&]() __attribute__((always_inline)) {
    xso += x_step;
    if (++xk == S) {
      xk = 0;
      ++xi;
      x_setup();
    }
  };
  // raw fp32 pairs (frames 2 c, 2 c + 1 of channel 8 q + j) of the two K-steps behind the one in use, and the B fragments
  // [column block][plane] of the step in use and of the next one
  f32x2v raw[2][8];
  x8 bq[2][2][2];
  auto x_load = [&](auto slot_c, auto j_c, auto n_c) __attribute__((always_inline)) {  // loads j0 .. j0 + n - 1 of the step at (xi, xk)
    constexpr int s = decltype(slot_c)::value, j0 = decltype(j_c)::value, nj = decltype(n_c)::value;
#pragma unroll
    for (int j = j0; j < j0 + nj; ++j) {  // (operands through locals: clang does not capture a variable that a generic
      const int so = xso + j * row_b, vo = x_voff;  // lambda names in asm operands only)
      const u32x4v rs = xr;
      if constexpr (R16) {  // two bf16 frames in one word (kept in element 0 of the slot's pair)
        float out;
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(out) : "v"(vo), "s"(rs), "s"(so) : "memory");
        raw[s][j][0] = out;
      } else {
        f32x2v out;
        asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(out) : "v"(vo), "s"(rs), "s"(so) : "memory");
        raw[s][j] = out;
      }
    }
  };
  auto x_load8 = [&](auto slot_c) __attribute__((always_inline)) { x_load(slot_c, bic<0>{}, bic<8>{}); };
  // counted wait; names the registers of the step that is consumed next, so that no use is scheduled above it
  auto x_wait = [&](auto slot_c, auto n_c) __attribute__((always_inline)) {
    constexpr int s = decltype(slot_c)::value, n = decltype(n_c)::value;
    f32x2v(&q)[8] = raw[s];
    asm volatile("s_waitcnt vmcnt(%8)"
                 : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7])
                 : "n"(n)
                 : "memory");
  };

  // ---- weights: LDS-DMA, eight pieces per wave and K-step: (plane 0 | 1, k-quarter 0..3) of rows 64 wave .. + 63 ----------
  const int w_voff = lane * 32;  // byte offset of (row lane, k 0) inside a 64-row group of the packer's [row][16 k] image
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.wt), 0, a.tiles_m * a.ksteps * 16384, 0x00020000);
  const int a_src = hw * 2048;  // source, per 16-k slot: [plane][256 rows][16 k]
  const int a_dst = hw * 1024;  // image: [plane][k-quarter][256 rows][8 k]
  int ai = lo, ak = 0, aso = 0;
  auto a_setup = [&]() __attribute__((always_inline)) {
    int n, mt, tt;
    decode(ai, n, mt, tt);
    aso = ai < hi ? mt * a.ksteps * 16384 + a_src : 0x7f000000;  // past the end: outside the descriptor
#ifdef PS_PP_STAMPS
    if (a.ablate & 2) aso = 0x7f000000;
#endif
  };
  auto dma_a1 = [&](int slot, auto i_c) __attribute__((always_inline)) {  // piece i = 4 plane + k-quarter
    constexpr int pl = decltype(i_c)::value >> 2, kq = decltype(i_c)::value & 3;
    float* dst = reinterpret_cast<float*>(smem + slot * L::A_SLOT + a_dst + pl * 16384 + kq * 4096);
    // (everything into the scalar offset: an immediate offset would be added to the LDS address as well)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, dst, 16, w_voff, aso + pl * 8192 + (kq >> 1) * 16384 + (kq & 1) * 16, 0, 0);
  };
  auto a_advance = [&]() __attribute__((always_inline)) {
    aso += 2 * 16384;
    if (++ak == S) {
      ak = 0;
      ++ai;
      a_setup();
    }
  };

  auto bias_dma = [&](int n, int mt, int par) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t br = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.bias ? a.bias : a.x), 0, a.bias ? (LN ? 128 : a.M) * 4 : 0, 0x00020000);  // (LN: 128 real rows)
    const __amdgpu_buffer_rsrc_t bnr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.bias_n ? a.bias_n + (size_t)n * a.M : a.x), 0, a.bias_n ? a.M * 4 : 0, 0x00020000);
    float* dst = bias_lds + par * 2 * XB_M;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(br, dst, 16, lane * 16, mt * XB_M * 4, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(bnr, dst + XB_M, 16, lane * 16, mt * XB_M * 4, 0, 0);
  };

  // ---- transform + split of one K-step in registers: raw slot -> the B fragments of that step -------------------------------
  int si = lo, sk = 0, spar = 0;  // supertile, step, bias-table parity of the step transformed next
  const float* stab = tab + 8 * lq;
  float sxs = xs_u[0];  // no prologue: scale of the utterance being transformed
  auto s_setup = [&]() __attribute__((always_inline)) {
    int n, mt, tt;
    decode(si, n, mt, tt);
    stab = tab + (n - n_lo) * 1024 + 8 * lq;
    sxs = n == n_lo ? xs_u[0] : xs_u[1];
    if (hw == 0 && si < hi) bias_dma(n, mt, spar);
  };
  auto s_advance = [&]() __attribute__((always_inline)) {
    stab += L::KS;
    if (++sk == S) {
      sk = 0;
      ++si;
      spar ^= 1;
      s_setup();
    }
  };
  f32x2v tsc, tsh;  // scale / shift of the row pair transformed next (read one chunk ahead: four registers, not sixteen)
  auto T_tab = [&](auto p_c) __attribute__((always_inline)) {
    constexpr int j = 2 * decltype(p_c)::value;
    if constexpr (TR) {
      tsc = *reinterpret_cast<const f32x2v*>(stab + j);
      tsh = *reinterpret_cast<const f32x2v*>(stab + 512 + j);
    }
  };
  float sv[4];  // channels j, j + 1 of the row pair in work, both frames: [j f0, j f1, j+1 f0, j+1 f1]
  // (The transform is pure arithmetic: nothing but its operands holds it in its chunk -- left alone, instruction selection
  //  gathers all of it right behind the wait that delivers the raw values.  Empty asm statements take the values in and out.)
  auto T_tr = [&](auto slot_c, auto p_c) __attribute__((always_inline)) {  // row pair p of the slot: transform
    constexpr int s = decltype(slot_c)::value, j = 2 * decltype(p_c)::value;
    {
      f32x2v &r0 = raw[s][j], &r1 = raw[s][j + 1];
      asm volatile("" : "+v"(r0), "+v"(r1));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int jj = j + (e >> 1);
      float v;
      if constexpr (R16) {
        const unsigned w = __builtin_bit_cast(unsigned, raw[s][jj][0]);
        v = __builtin_bit_cast(float, (e & 1) ? (w & 0xffff0000u) : (w << 16));
      } else {
        v = raw[s][jj][e & 1];
      }
      if constexpr (TR)
        sv[e] = prelu(v * tsc[e >> 1] + tsh[e >> 1], slope);
      else
        sv[e] = v * sxs;
    }
    {
      float &v0 = sv[0], &v1 = sv[1], &v2 = sv[2], &v3 = sv[3];
      asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
    }
  };
  auto T_split = [&](auto slot_c, auto p_c) __attribute__((always_inline)) {  // row pair p: two fp16 terms, both frames
    constexpr int s = decltype(slot_c)::value, j = 2 * decltype(p_c)::value;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float v0 = sv[cb], v1 = sv[2 + cb];  // channels j, j + 1 of frame 2 c + cb
      const x2 hh = __builtin_convertvector(f32x2v{v0, v1}, x2);
      bq[s][cb][0][j] = hh[0];
      bq[s][cb][0][j + 1] = hh[1];
      if constexpr (!R16) {
        const f32x2v back = __builtin_convertvector(hh, f32x2v);
        v0 -= back[0];
        v1 -= back[1];
        const x2 ll = __builtin_convertvector(f32x2v{v0, v1}, x2);
        bq[s][cb][1][j] = ll[0];
        bq[s][cb][1][j + 1] = ll[1];
      }
    }
  };
  auto T_pin = [&](auto slot_c) __attribute__((always_inline)) {
    constexpr int s = decltype(slot_c)::value;
    if constexpr (R16) {
      x8 &b0 = bq[s][0][0], &b2 = bq[s][1][0];
      asm volatile("" : "+v"(b0), "+v"(b2));
    } else {
      x8 &b0 = bq[s][0][0], &b1 = bq[s][0][1], &b2 = bq[s][1][0], &b3 = bq[s][1][1];
      asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
    }
  };

  // ---- compute side: acc[rb][cb][r] = row 16 rb + 4 lq + r, frame t0 + 32 hw + 2 lc + cb ---------------------------------------
  f32x4 acc[16][2];
  const int lane_off = (4 * lq * a.ldt + 2 * lc) * ES;
  auto init_acc = [&](int idx) __attribute__((always_inline)) {
    if constexpr (RES) {
      int n, mt, tt;
      decode(idx, n, mt, tt);
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
          reinterpret_cast<unsigned char*>(const_cast<float*>(a.res)) + (size_t)n * a.M * a.ldt * ES, 0,
          idx < hi ? a.M * a.ldt * ES : 0, 0x00020000);
      const int tile_off = (mt * XB_M * a.ldt + tt * XB_T + hw * 32) * ES;
#pragma unroll
      for (int rb = 0; rb < 16; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (R16) {
            const unsigned w = __builtin_amdgcn_raw_buffer_load_b32(rr, lane_off, tile_off + (rb * 16 + r) * row_b, 0);
            acc[rb][0][r] = __builtin_bit_cast(float, w << 16);
            acc[rb][1][r] = __builtin_bit_cast(float, w & 0xffff0000u);
          } else {
            const f32x2v v = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(rr, lane_off, tile_off + (rb * 16 + r) * row_b, 0));
            acc[rb][0][r] = v[0];
            acc[rb][1][r] = v[1];
          }
        }
    } else {
#pragma unroll
      for (int rb = 0; rb < 16; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rb][0][r] = 0.f, acc[rb][1][r] = 0.f;
    }
  };
  // with a residual the accumulators count in scaled units (2^(w_exp + x_exp)): the residual they start from is brought
  // there too (a power of two: exact) once its loads have landed
  auto scale_res = [&](int idx) __attribute__((always_inline)) {
    if constexpr (RES) {
      int n, mt, tt;
      decode(idx, n, mt, tt);
      const float inv = 1.f / (n == n_lo ? os_u[0] : os_u[1]);
#pragma unroll
      for (int rb = 0; rb < 16; ++rb) acc[rb][0] *= inv, acc[rb][1] *= inv;
    }
  };
  auto acc_fence = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int rb = 0; rb < 16; rb += 4)
      asm volatile("" : "+v"(acc[rb][0]), "+v"(acc[rb][1]), "+v"(acc[rb + 1][0]), "+v"(acc[rb + 1][1]), "+v"(acc[rb + 2][0]),
                   "+v"(acc[rb + 2][1]), "+v"(acc[rb + 3][0]), "+v"(acc[rb + 3][1]));
  };

  const unsigned char* const a_frag = smem + lq * 4096 + lc * 16;  // + slot * A_SLOT + plane * 16384 + rb * 256
#ifndef RB_PACE
#define RB_PACE 0
#endif
#ifndef RB_AD
#define RB_AD 2  // row blocks the A-fragment reads run ahead of the MFMAs (8 registers each)
#endif
  constexpr int AD = RB_AD, AF = AD + 1;
  x8 af[AF][2];  // [rb % AF][plane]
  auto read_afrags = [&](int sa, auto rb_c) __attribute__((always_inline)) {
    constexpr int rb = decltype(rb_c)::value;
    if constexpr (!R16) af[rb % AF][1] = *reinterpret_cast<const x8*>(a_frag + sa + 16384 + rb * 256);  // (in the order of use)
    af[rb % AF][0] = *reinterpret_cast<const x8*>(a_frag + sa + rb * 256);
  };
  // the three products of one row block on both column blocks, smallest terms first: (W1, x0), (W0, x1), (W0, x0)
  auto mf_block = [&](auto rb_c, auto s_c) __attribute__((always_inline)) {
    constexpr int rb = decltype(rb_c)::value, s = decltype(s_c)::value;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      if constexpr (!R16) {
        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb % AF][1], bq[s][cb][0], acc[rb][cb], 0, 0, 0);
        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb % AF][0], bq[s][cb][1], acc[rb][cb], 0, 0, 0);
      }
      acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb % AF][0], bq[s][cb][0], acc[rb][cb], 0, 0, 0);
    }
  };

  // finished tile of supertile idx: scale, bias, statistics, maxima, stores; then the accumulators take the residual of
  // the wave's next tile
  auto drain = [&](int idx, int parity) __attribute__((always_inline)) {
    int n, mt, tt, nn, nmt, ntt;
    decode(idx, n, mt, tt);
    decode(idx + 1, nn, nmt, ntt);
    const int m0 = mt * XB_M, t0 = tt * XB_T + hw * 32;
    float fsum = 0.f, fsq = 0.f, amx0 = 0.f, amx1 = 0.f;
    const float osc = n == n_lo ? os_u[0] : os_u[1];
    const int slab = (FM ? a.fm_ld : a.M) * a.ldt * ES;
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<unsigned char*>(a.y) + (size_t)n * (FM ? a.fm_ld : a.M) * a.ldt * ES, 0, slab, 0x00020000);
    const int tile_off = (m0 * a.ldt + t0) * ES;
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<unsigned char*>(const_cast<float*>(RES ? a.res : a.y)) + (size_t)nn * a.M * a.ldt * ES, 0,
        (RES && idx + 1 < hi) ? slab : 0, 0x00020000);
    [[maybe_unused]] const int ntile_off = (nmt * XB_M * a.ldt + ntt * XB_T + hw * 32) * ES;
    const bool cm0 = t0 + 2 * lc < a.T, cm1 = t0 + 2 * lc + 1 < a.T;  // (selects, not 0/1 factors: 0 * NaN would poison the sums)
    const float* bl = bias_lds + parity * 2 * XB_M + 4 * lq;
    if constexpr (LN) {
      // y[c][frame] = res[c][frame] + LayerNorm_c(W f(x) + b)[c], or LayerNorm_c(W f(x) + b + res) with ln_inside, c < 128
      // (ps_conv1x1_f16x2_ln_f32: the projection + LayerNorm + skip behind a recurrence, dpcrn.py:56-80; the post-norm blocks of
      // MhaSelfAttenLayer, lobe/attention.py:202-232).  The tile holds every channel of its frames: rows 16 rb + 4 lq + r, rb < 8, of
      // frame 2 lc + cb sit in the four lanes lq of column lc -- two cross-lane adds per statistic; two-pass variance as
      // nn.LayerNorm.  (The weight image is zero padded to 256 rows: the upper eight row blocks compute zeros.)
      const int cslab = 128 * a.ldt * 4;
      const __amdgpu_buffer_rsrc_t yl = __builtin_amdgcn_make_buffer_rsrc(
          reinterpret_cast<unsigned char*>(a.y) + (size_t)n * cslab, 0, cslab, 0x00020000);
      const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(
          reinterpret_cast<unsigned char*>(const_cast<float*>(a.res)) + (size_t)n * cslab, 0, a.res ? cslab : 0, 0x00020000);
      const int toff = t0 * 4;
      f32x2v resv[8][4];
#pragma unroll
      for (int rb = 0; rb < 8; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          resv[rb][r] = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(rl, lane_off, toff + (rb * 16 + r) * row_b, 0));
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int rb = 0; rb < 8; ++rb) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(bl + rb * 16) + *reinterpret_cast<const f32x4*>(bl + XB_M + rb * 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[rb][0][r] = acc[rb][0][r] * osc + b4[r];
          acc[rb][1][r] = acc[rb][1][r] * osc + b4[r];
          if (a.ln_inside) {  // (uniform) post-norm form: the residual joins in front of the norm
            acc[rb][0][r] += resv[rb][r][0];
            acc[rb][1][r] += resv[rb][r][1];
            resv[rb][r] = f32x2v{0.f, 0.f};
          }
          s0 += acc[rb][0][r];
          s1 += acc[rb][1][r];
        }
      }
      s0 += __shfl_xor(s0, 16), s1 += __shfl_xor(s1, 16);
      s0 += __shfl_xor(s0, 32), s1 += __shfl_xor(s1, 32);
      const float mean0 = s0 * (1.f / 128.f), mean1 = s1 * (1.f / 128.f);
      float q0 = 0.f, q1 = 0.f;
#pragma unroll
      for (int rb = 0; rb < 8; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d0 = acc[rb][0][r] - mean0, d1 = acc[rb][1][r] - mean1;
          q0 += d0 * d0;
          q1 += d1 * d1;
        }
      q0 += __shfl_xor(q0, 16), q1 += __shfl_xor(q1, 16);
      q0 += __shfl_xor(q0, 32), q1 += __shfl_xor(q1, 32);
      const float rstd0 = 1.f / sqrtf(q0 * (1.f / 128.f) + a.ln_eps), rstd1 = 1.f / sqrtf(q1 * (1.f / 128.f) + a.ln_eps);
#pragma unroll
      for (int rb = 0; rb < 8; ++rb) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.ln_gamma + rb * 16 + 4 * lq);
        const f32x4 e4 = *reinterpret_cast<const f32x4*>(a.ln_beta + rb * 16 + 4 * lq);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v0 = (acc[rb][0][r] - mean0) * rstd0 * g4[r] + e4[r] + resv[rb][r][0];
          const float v1 = (acc[rb][1][r] - mean1) * rstd1 * g4[r] + e4[r] + resv[rb][r][1];
          asm volatile("v_max_f32 %0, %0, |%1|" : "+v"(amx0) : "v"(v0));
          asm volatile("v_max_f32 %0, %0, |%1|" : "+v"(amx1) : "v"(v1));
          __builtin_amdgcn_raw_buffer_store_b64(u32x2v{__builtin_bit_cast(unsigned, v0), __builtin_bit_cast(unsigned, v1)}, yl,
                                                lane_off, toff + (rb * 16 + r) * row_b, 0);
        }
      }
#pragma unroll
      for (int rb = 0; rb < 16; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rb][0][r] = 0.f, acc[rb][1][r] = 0.f;
    } else if constexpr (FM) {
      // frame-major output y[n][frame][fm_ld >= M] (ps_conv1x1_f16x2_fmajor_f32: the gate pre-activations of ps_lstm_fmajor_f16x2_f32):
      // the lane's four rows 16 rb + 4 lq .. + 3 are 16 consecutive bytes of its frame.
      // Whole 128-byte lines per store instruction: the four lanes lq of a column hold 64 bytes of a frame per row block, so
      // column c and column c ^ 8 swap halves (v_mov_dpp row_ror:8, the columns are the 16 lanes of a DPP row) -- the low
      // column stores row block 2j of both frames, the high column row block 2j + 1 -- and an instruction covers 8 frames x
      // 128 bytes instead of 16 x 64 (64-byte pieces: 1.43 ms per launch against 1.06 for the channel-major epilogue).
      const bool low = lc < 8;
      const int hi64 = low ? 0 : 64;
      const int v1 = (2 * (lc & 7) * a.fm_ld + 4 * lq) * 4 + hi64, v2 = (2 * (lc | 8) * a.fm_ld + 4 * lq) * 4 + hi64;
      const int fm_tile = (t0 * a.fm_ld + m0) * 4;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f32x4 o[2][2];  // [row block 2j + i][frame cb]
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int rb = 2 * j + i;
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(bl + rb * 16) + *reinterpret_cast<const f32x4*>(bl + XB_M + rb * 16);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            o[i][0][r] = acc[rb][0][r] * osc + b4[r];
            o[i][1][r] = acc[rb][1][r] * osc + b4[r];
            asm volatile("v_max_f32 %0, %0, |%1|" : "+v"(amx0) : "v"(o[i][0][r]));
            asm volatile("v_max_f32 %0, %0, |%1|" : "+v"(amx1) : "v"(o[i][1][r]));
            acc[rb][0][r] = 0.f, acc[rb][1][r] = 0.f;
          }
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          f32x4 recv;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float send = low ? o[1][cb][r] : o[0][cb][r];
            recv[r] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0x128, 0xf, 0xf, false));
          }
          f32x4 d1, d2;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            d1[r] = low ? o[0][cb][r] : recv[r];
            d2[r] = low ? recv[r] : o[1][cb][r];
          }
          const int so = fm_tile + cb * a.fm_ld * 4 + j * 128;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, d1), yr, v1, so, PS_FM_AUX);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, d2), yr, v2, so, PS_FM_AUX);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
    for (int rb = 0; rb < 16; ++rb) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(bl + rb * 16) + *reinterpret_cast<const f32x4*>(bl + XB_M + rb * 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v0 = acc[rb][0][r] * osc + b4[r], v1 = acc[rb][1][r] * osc + b4[r];
        asm volatile("v_max_f32 %0, %0, |%1|" : "+v"(amx0) : "v"(v0));
        asm volatile("v_max_f32 %0, %0, |%1|" : "+v"(amx1) : "v"(v1));
        if constexpr (STATS) {
          const float m0v = cm0 ? v0 : 0.f, m1v = cm1 ? v1 : 0.f;
          fsum += m0v;
          fsq += m0v * m0v;
          fsum += m1v;
          fsq += m1v * m1v;
        }
        const int ro = (rb * 16 + r) * row_b;
        if constexpr (R16) {
          const bf16x2 pk = __builtin_convertvector(f32x2v{v0, v1}, bf16x2);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, pk), yr, lane_off, tile_off + ro, 0);
        } else {
          __builtin_amdgcn_raw_buffer_store_b64(u32x2v{__builtin_bit_cast(unsigned, v0), __builtin_bit_cast(unsigned, v1)}, yr,
                                                lane_off, tile_off + ro, 0);
        }
        if constexpr (RES && R16) {
          const unsigned w = __builtin_amdgcn_raw_buffer_load_b32(rr, lane_off, ntile_off + ro, 0);
          acc[rb][0][r] = __builtin_bit_cast(float, w << 16);
          acc[rb][1][r] = __builtin_bit_cast(float, w & 0xffff0000u);
        } else if constexpr (RES) {
          const f32x2v nv = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(rr, lane_off, ntile_off + ro, 0));
          acc[rb][0][r] = nv[0];
          acc[rb][1][r] = nv[1];
        } else {
          acc[rb][0][r] = 0.f, acc[rb][1][r] = 0.f;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#if RB_PACE > 0
      // pacing: at most RB_PACE row blocks of this wave's drain traffic in flight.  The CU's memory path serves requests
      // in order, so the other workgroup's activation loads (8 per K-step) would otherwise queue behind a whole tile's
      // stores and residual loads (512 KiB per workgroup for out_conv)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(RB_PACE * (RES ? 8 : 4)) : "memory");
#endif
    }
    }
    if constexpr (STATS) {
      const double s = wave_sum_dpp(fsum), q = wave_sum_dpp(fsq);
      if (lane == 0) {
        const int parts = a.tiles_m * a.tiles_t * 4;
        const int part = (mt * a.tiles_t + tt) * 4 + hw;
        double* dst = a.ostats + ((size_t)n * parts + part) * 2;
        dst[0] = s;
        dst[1] = q;
      }
    }
    if (a.y_amax) {
      const float m = wave_max(fmaxf(cm0 ? amx0 : 0.f, cm1 ? amx1 : 0.f));
      if (lane == 0) a.y_amax[(size_t)n * (a.tiles_m * a.tiles_t * 4) + (mt * a.tiles_t + tt) * 4 + hw] = m;
    }
  };

  // ---- prologue: x(0), then the issue order of the "intervals" -2, -1 so that the counted wait holds from g = 0 --------------
  if (a.delay > 0 && (int)blockIdx.x >= a.groups) {  // the second half of the grid starts `delay` cycles late (see the header)
    unsigned long long t_start, now;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_start)::"memory");
    const unsigned long long until = t_start + (unsigned long long)a.delay;
    do {
      __builtin_amdgcn_s_sleep(32);
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
    } while (now < until);
  }
  x_setup();
  a_setup();
  x_load8(bic<0>{});
  x_advance();
  if (hw == 0) bias_dma(n_lo, mt_lo, 0);
  init_acc(lo);
  acc_fence();
  scale_res(lo);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  x_wait(bic<0>{}, bic<0>{});
  __syncthreads();  // the prologue tables are in LDS
  T_tab(bic<0>{}), T_tr(bic<0>{}, bic<0>{}), T_split(bic<0>{}, bic<0>{});
  T_tab(bic<1>{}), T_tr(bic<0>{}, bic<1>{}), T_split(bic<0>{}, bic<1>{});
  T_tab(bic<2>{}), T_tr(bic<0>{}, bic<2>{}), T_split(bic<0>{}, bic<2>{});
  T_tab(bic<3>{}), T_tr(bic<0>{}, bic<3>{}), T_split(bic<0>{}, bic<3>{});
  T_pin(bic<0>{});
  stab += L::KS, sk = 1;  // (S >= 2: step 1 belongs to the same supertile)
  // "intervals" -2, -1: A(v + 1) early, x(v + 3) late
  x_load8(bic<1>{});
  x_advance();
  dma_a1(0, bic<0>{}), dma_a1(0, bic<1>{}), dma_a1(0, bic<2>{}), dma_a1(0, bic<3>{});
  if constexpr (!R16) dma_a1(0, bic<4>{}), dma_a1(0, bic<5>{}), dma_a1(0, bic<6>{}), dma_a1(0, bic<7>{});
  a_advance();
  x_load8(bic<0>{});
  x_advance();
  x_wait(bic<1>{}, bic<VMW>{});  // A(0) and x(1) have landed
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  read_afrags(0, bic<0>{});
  if constexpr (AD == 2) read_afrags(0, bic<1>{});

#ifdef PS_PP_STAMPS
  unsigned long long rb_t0 = 0, rb_rt0 = 0, rb_d = 0;
  if (a.stamps) {
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rb_rt0)::"memory");  // constant 100 MHz
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rb_t0)::"memory");
  }
#endif
  // ---- main loop, two intervals per trip.  Interval g: 16 x [A fragments of row block rb + 1 | 6 MFMAs of row block rb |
  // chunk rb of the side work: weight DMA, transform of x(g+1), loads of x(g+3) into the slot it leaves]; first fragments
  // of step g + 1; counted wait; barrier; a finished tile's drain ---------------------------------------------------------
  int ci = lo, ck = 0, parity = 0;
  auto interval = [&](auto u_c) __attribute__((always_inline)) {
    constexpr int u = decltype(u_c)::value;  // g & 1: fragment set of step g, raw slot of x(g+2) (waited for)
    constexpr int s1 = u ^ 1;                // fragment set / raw slot of x(g+1) (transformed now), then of x(g+3)
    constexpr int sa = u * L::A_SLOT;  // weight slot of step g; A(g+1) goes to the other one, free since the last barrier
    auto chunk = [&](auto c_c) __attribute__((always_inline)) {
      constexpr int c = decltype(c_c)::value;
      if constexpr (c < 4 && !R16) dma_a1(s1, bic<2 * c>{}), dma_a1(s1, bic<2 * c + 1>{});
      if constexpr (c < 4 && R16) dma_a1(s1, bic<c>{});  // (the first fp16 term of the weights only)
      if constexpr (c == 3) T_tab(bic<0>{});
      if constexpr (c >= 4 && c < 12 && (c & 1) == 0) T_tr(bic<s1>{}, bic<(c - 4) / 2>{});
      if constexpr (c >= 4 && c < 12 && (c & 1) == 1) T_split(bic<s1>{}, bic<(c - 4) / 2>{});
      if constexpr (c == 5 || c == 7 || c == 9) T_tab(bic<(c - 3) / 2>{});
      if constexpr (c == 11) T_pin(bic<s1>{});
      if constexpr (c >= 12) x_load(bic<s1>{}, bic<2 * (c - 12)>{}, bic<2>{});
    };
    auto slot = [&](auto rb_c) __attribute__((always_inline)) {
      constexpr int rb = decltype(rb_c)::value;
      if constexpr (rb + AD < 16) read_afrags(sa, bic<(rb + AD) % 16>{});
      __builtin_amdgcn_sched_barrier(0);
#ifdef PS_PP_STAMPS  // (diagnostic build: ps_debug_ablate 1 / 4 removes the MFMAs / the chunks)
      const bool do_chunk = !(a.ablate & 4);
      if (!(a.ablate & 1))
#else
      constexpr bool do_chunk = true;
#endif
        mf_block(rb_c, bic<u>{});
      __builtin_amdgcn_sched_barrier(0);
      if (do_chunk) chunk(rb_c);
      __builtin_amdgcn_sched_barrier(0);
    };
    slot(bic<0>{}), slot(bic<1>{}), slot(bic<2>{}), slot(bic<3>{});
    slot(bic<4>{}), slot(bic<5>{}), slot(bic<6>{}), slot(bic<7>{});
    slot(bic<8>{}), slot(bic<9>{}), slot(bic<10>{}), slot(bic<11>{});
    slot(bic<12>{}), slot(bic<13>{}), slot(bic<14>{}), slot(bic<15>{});
    a_advance();
    x_advance();
    s_advance();
    x_wait(bic<u>{}, bic<VMW>{});  // this wave's pieces of A(g+1) and its x(g+2) have landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (ck == S - 1 && ci < hi) {
#ifdef PS_PP_STAMPS
      unsigned long long d0 = 0, d1 = 0;
      if (a.stamps) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(d0)::"memory");
#endif
      drain(ci, parity);
      parity ^= 1;
      acc_fence();  // the wait for the residual loads belongs here, not in front of every iteration's MFMAs
      if (ci + 1 < hi) scale_res(ci + 1);
#ifdef PS_PP_STAMPS
      if (a.stamps) {
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(d1)::"memory");
        rb_d += d1 - d0;
      }
#endif
    }
    if (++ck == S) {
      ck = 0;
      ++ci;
    }
    read_afrags(s1 * L::A_SLOT, bic<0>{});  // first fragments of step g + 1
    if constexpr (AD == 2) read_afrags(s1 * L::A_SLOT, bic<1>{});
  };
  for (int g = 0; g < total; g += 2) {  // (a step past `total` runs on empty descriptors and drains nothing)
    interval(bic<0>{});
    interval(bic<1>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing of this workgroup's is in flight when it leaves
#ifdef PS_PP_STAMPS
  if (a.stamps && tid == 0) {  // the layout tools/time_f16x2.py reads (one record per workgroup here: 512 records)
    unsigned long long now, rnow;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rnow)::"memory");
    unsigned long long* d = a.stamps + (size_t)blockIdx.x * 6;
    d[0] = now - rb_t0;
    d[1] = 0;
    d[2] = rnow - rb_rt0;  // 10 ns units: d[0] / d[2] / 10 = the clock the kernel ran at, in GHz
    d[3] = 0;
    d[4] = rb_d;
    d[5] = (unsigned long long)(2 * total);  // in 16-deep steps, the unit of the other kernels' records
  }
#endif
}
