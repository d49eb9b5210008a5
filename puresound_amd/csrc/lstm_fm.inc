// ---- H = 128, 16 sequences per workgroup, fp16x2 recurrent product, frame-major pre-activations -----------------------
// (ps_lstm_fmajor_f16x2_f32; included by rnn.hip inside namespace ps)
//
// The bottleneck LSTMs of DPCRN (dpcrn.py:34-81 of mcw519/PureSound) at 32 x 4 s: 32,064 sequences of 64 steps in both
// directions along frequency, then 2,048 sequences of 501 steps along time, H = 128.  On lstm_m4_kernel (4 sequences per
// workgroup, fp32 4x4x1 MFMA) they take 4.15 ms and 2.9 ms per pass (profiles/r04_dpcrn_kernels_before.txt): the fp32
// matrix pipe is the floor of the first (269 GFLOP per pass at 157 TFLOP/s = 1.7 ms), and the second fetches every
// 128-byte line of its channel-major gate rows eight times (a lane reads 16 bytes of a line every 4 steps, 2,048 x 512
// lines in flight against 32 MB of L2).
//
// Here  * the recurrent product runs as v_mfma_f32_16x16x32_f16 on two fp16 terms per operand (the scheme of
//         lstm_seg_f16x2_kernel: W_hh 2^e = W_hi + W_lo once, h 2^10 = h_hi + h_lo every step, three products, fp32
//         accumulation on top of the scaled fp32 pre-activations): 48 issues = 768 matrix-pipe cycles per wave and step for
//         16 sequences, against 128 x 8 = 1,024 for 4;
//       * the pre-activations are FRAME-MAJOR, gx [N][ldt][D*4H] (ps_conv1x1_f16x2_fmajor_f32 writes them so): the 4 x 16
//         bytes a lane needs for a step are the gates (i, f, g, o) of its 4 units at its sequence's frame, every fetched
//         byte is used, and in both passes a workgroup's step is 16 runs of 2 KiB;
//       * they reach LDS by DMA (buffer_load_dwordx4 ... lds), PF = 4 steps ahead, into a ring [slot][wave][gate][lane] that
//         each wave fills and reads for itself -- no registers held across the flight, no barrier for the ring; the wait is
//         a counted s_waitcnt vmcnt (loads, stores and LDS-DMA retire in issue order; counts derived at NW below);
//       * a workgroup is persistent: it walks blocks of 16 sequences (never across utterances, so a 32-bit buffer offset
//         covers a block's utterance), the DMA stream running on into the next block's first steps.
// Wave w owns units 16 w .. 16 w + 15: A fragments (W_hi, W_lo: 128 VGPRs) resident; lane (col = lane & 15, quad = lane >>
// 4) holds after the MFMAs gate g of units 16 w + 4 quad + r (r = 0..3) of sequence col in acc[g][r] and does their
// cell update alone; h' crosses LDS as [plane][sequence][k] halves (8-byte writes, 16-byte reads, rows of H + 8 halves:
// conflict-free), double buffered, one barrier per step.
struct LstmFm {
  ps_lstm_args a;
  int ldm;    // floats between consecutive frames of gx (>= D*4H)
  int ablate; // profiling only (ps_debug_ablate): 1 = no h' stores
  int nblk;   // blocks of 16 sequences per utterance
  int total;  // N * nblk
};

template <bool CONTIG>
__global__ __launch_bounds__(512, 1) void lstm_fm_f16x2_kernel(LstmFm k) {
  constexpr int H = 128, G = 4 * H, PF = 4, LDK = H + 8;
  __shared__ __attribute__((aligned(16))) unsigned char ring[PF * 8 * 4 * 1024];
  __shared__ __attribute__((aligned(16))) _Float16 hb[2][2][16][LDK];
  __shared__ float wmax[8];
  const ps_lstm_args& a = k.a;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, quad = lane >> 4;
  const int d = blockIdx.z;
  const bool rev = d == 1;
  const int Mtot = k.ldm;  // (frame stride)
  const int unit0 = 16 * w + 4 * quad;
  const int steps = a.steps;
  const int SP = CONTIG ? (steps + 3) / 4 * 4 : steps;  // steps walked per block (CONTIG: whole 16-byte groups)
  // blocks sharing 128-byte lines of hout (neighbours along q) go to one XCD: id -> (id % 8) * (grid / 8) + id / 8
  const int per = gridDim.x >> 3;
  const int wg = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const int niter = (k.total + (int)gridDim.x - 1) / (int)gridDim.x;

  // ---- recurrent weights: maximum, scale, two fp16 terms --------------------------------------------------------------------
  // A fragment of gate g, k-step ks: lane (row = lane & 15 -> unit 16 w + row, k-group = lane >> 4) holds k = 32 ks + 8 kgroup + e
  const float* wt = a.whh_t + (size_t)d * H * G;
  f16x8 whi[4][4], wlo[4][4];
  float inv, up;
  {
    float m = 0.f;
    for (int g = 0; g < 4; ++g)
      for (int kk = 0; kk < 32; ++kk) m = fmaxf(m, fabsf(wt[(size_t)(32 * (kk >> 3) + 8 * quad + (kk & 7)) * G + g * H + 16 * w + col]));
    m = wave_max(m);
    if (lane == 0) wmax[w] = m;
    __syncthreads();
    m = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmaxf(m, wmax[i]);
    int ex = 0;
    if (m > 0.f) frexpf(m, &ex);  // m = f * 2^ex, f in [0.5, 1)
    ex = ex < -27 ? -27 : ex;     // (tiny matrices: keep the scaled products far from overflow)
    const float S = ldexpf(1.f, 13 - ex);
    up = S * 1024.f;              // scale of the accumulators: (W 2^(13-ex)) (h 2^10)
    inv = 1.f / up;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float ws = wt[(size_t)(32 * ks + 8 * quad + e) * G + g * H + 16 * w + col] * S;
          const _Float16 hi = (_Float16)ws;
          whi[g][ks][e] = hi;
          wlo[g][ks][e] = (_Float16)(ws - (float)hi);
        }
  }

  // ---- block cursors ----------------------------------------------------------------------------------------------------------
  // block `it` of this workgroup: utterance n (uniform), the lane's sequence q; gx byte offset of (sequence, d, unit0) inside
  // the utterance's slab; hout byte offset inside the (n, d) slab, out of range for a lane past the last sequence (the
  // buffer store is then dropped: no branch around the stores, whose count the wait below relies on)
  const unsigned slab_g = (unsigned)a.ldt * Mtot * 4u, slab_h = (unsigned)H * a.ldt * 4u;
  auto decode = [&](int it, int& n, int& gvoff, int& hvoff) __attribute__((always_inline)) {
    int b = it * (int)gridDim.x + wg;
    b = b < k.total ? b : k.total - 1;
    n = __builtin_amdgcn_readfirstlane(b / k.nblk);
    const int q = (b % k.nblk) * 16 + col;
    const int qq = q < a.Q ? q : a.Q - 1;
    gvoff = (qq * a.q_stride * Mtot + d * G + unit0) * 4;
    hvoff = q < a.Q ? (unit0 * a.ldt + q * a.q_stride) * 4 : 0x7ffffff0;
  };
  auto gx_rsrc = [&](int n) __attribute__((always_inline)) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.gx) + (size_t)n * a.ldt * Mtot, 0, slab_g, 0x00020000);
  };

  // prefetch cursor: step pf_s of block pf_it (past the last block: its last step again, into a slot nobody reads)
  int pf_it = 0, pf_s = 0, pf_n, pf_gvoff, pf_dummy;
  decode(0, pf_n, pf_gvoff, pf_dummy);
  __amdgpu_buffer_rsrc_t pf_r = gx_rsrc(pf_n);
  int pf_slot = 0;
  auto dma_step = [&]() __attribute__((always_inline)) {
    const int sc = pf_s < steps ? pf_s : steps - 1;  // (CONTIG: the dead steps of the last group replay the last frame)
    const int ts = rev ? steps - 1 - sc : sc;
    const int so = ts * a.step_stride * Mtot * 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float* dst = reinterpret_cast<float*>(ring + ((pf_slot * 8 + w) * 4 + g) * 1024);
      // (everything into the scalar offset: an immediate offset would be added to the LDS address as well)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(pf_r, dst, 16, pf_gvoff, so + g * H * 4, 0, 0);
    }
    pf_slot = pf_slot == PF - 1 ? 0 : pf_slot + 1;
    if (++pf_s == SP) {
      pf_s = 0;
      if (pf_it + 1 < niter) {
        ++pf_it;
        decode(pf_it, pf_n, pf_gvoff, pf_dummy);
        pf_r = gx_rsrc(pf_n);
      } else {
        pf_s = SP - 1;
      }
    }
  };

  auto put_h = [&](int buf, const float (&h)[4]) __attribute__((always_inline)) {  // 4 units of sequence col: two 8-byte writes
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

  const unsigned ring_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)ring;
  float c[4] = {0.f, 0.f, 0.f, 0.f}, h[4] = {0.f, 0.f, 0.f, 0.f};
  put_h(0, h);
  __syncthreads();  // (also: the weights' loads are all consumed -- no ordinary load is outstanding from here on)
#pragma unroll
  for (int i = 0; i < PF; ++i) dma_step();

  // Counted wait at the top of virtual step v for the DMA group of step v (issued PF steps earlier).  Younger operations at
  // that point: the DMA groups of steps v+1 .. v+PF-1 (4 each) and the h' stores issued since -- per step 4 dword stores
  // (PF steps' worth: 16), CONTIG one group of 4 16-byte stores per 4 steps (exactly one group in any PF = 4 consecutive
  // steps).  During the first PF steps fewer stores exist: 12 (the DMA groups alone) is exact for CONTIG and safe otherwise.
  constexpr int NW0 = 4 * (PF - 1), NW = CONTIG ? 4 * (PF - 1) + 4 : 4 * (PF - 1) + 4 * PF;
  int v = 0, buf = 0, slot = 0;
  for (int it = 0; it < niter; ++it) {
    int n, gv_unused, hvoff;
    decode(it, n, gv_unused, hvoff);
    const bool live = it * (int)gridDim.x + wg < k.total;  // uniform; a dead block (last iteration only) stores nothing
    const __amdgpu_buffer_rsrc_t hr = __builtin_amdgcn_make_buffer_rsrc(a.hout + (size_t)(n * a.D + d) * H * a.ldt, 0,
                                                                         (live && !(k.ablate & 1)) ? slab_h : 0, 0x00020000);
    float hst[4][4];
    for (int s0 = 0; s0 < SP; s0 += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int s = s0 + u;
        if (s < SP) {  // uniform (non-CONTIG: SP = steps need not be a multiple of 4)
          if (v < PF)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW0) : "memory");
          else
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW) : "memory");
          f32x4 acc[4];
          {
            // (inline asm: behind a compiler-visible LDS read the compiler puts an s_waitcnt vmcnt(0) -- "an LDS-DMA may
            //  be writing this" -- draining the whole prefetch every step; the counted wait above is the one that covers them)
            const unsigned ra = ring_lds + ((slot * 8 + w) * 4) * 1024 + lane * 16;
            asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\t"
                         "ds_read_b128 %3, %4 offset:3072"
                         : "=&v"(acc[0]), "=&v"(acc[1]), "=&v"(acc[2]), "=&v"(acc[3])
                         : "v"(ra)
                         : "memory");
          }
          f16x8 bh[2][4];
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) bh[pl][ks] = *reinterpret_cast<const f16x8*>(&hb[buf][pl][col][32 * ks + 8 * quad]);
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])::"memory");  // the slot is in registers: refill it
          dma_step();
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] *= up;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[g][ks], bh[0][ks], acc[g], 0, 0, 0);
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wlo[g][ks], bh[0][ks], acc[g], 0, 0, 0);
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[g][ks], bh[1][ks], acc[g], 0, 0, 0);
          const bool dead = CONTIG && s >= steps;  // uniform
          const int sc = s < steps ? s : steps - 1;
          const int ts = rev ? steps - 1 - sc : sc;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float gi = fast_sigmoid(acc[0][r] * inv);
            const float gf = fast_sigmoid(acc[1][r] * inv);
            const float gg = fast_tanh(acc[2][r] * inv);
            const float go = fast_sigmoid(acc[3][r] * inv);
            c[r] = gf * c[r] + gi * gg;
            h[r] = go * fast_tanh(c[r]);
            if constexpr (CONTIG) {
              hst[r][rev ? 3 - u : u] = dead ? 0.f : h[r];
            } else {
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, h[r]), hr, hvoff,
                                                    (ts * a.step_stride + r * a.ldt) * 4, 0);
            }
          }
          if (s == SP - 1) {  // the next block starts from zero states
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = 0.f, h[r] = 0.f;
          }
          put_h(buf ^ 1, h);
          if constexpr (CONTIG) {
            if (u == 3) {
              const int f0 = rev ? steps - 4 - s0 : s0;
#pragma unroll
              for (int r = 0; r < 4; ++r)
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(u32x4l, f32x4{hst[r][0], hst[r][1], hst[r][2], hst[r][3]}), hr, hvoff,
                    (f0 + r * a.ldt) * 4, 0);
            }
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          buf ^= 1;
          slot = slot == PF - 1 ? 0 : slot + 1;
          ++v;
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing DMA groups land before the LDS is released
}
