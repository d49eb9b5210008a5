// ---- H = 256 / 192, 16 sequences per workgroup, EXACT fp32 recurrent product, W_hh streamed from L2 -----------------------
// (ps_lstm_h256_f32; included by rnn.hip inside namespace ps)
//
// The fp32 arithmetic (set_gemm_precision("fp32")) of SkiM's 256-unit segment / Mem-LSTMs and of the 192-unit speaker LSTM ran
// on the generic lstm_kernel: a thread per gate row, 256 weights from L2 per thread and step, 4 sequences per workgroup.  This
// is lstm_fm_h256_kernel's work decomposition with the product W_hh h in v_mfma_f32_16x16x4_f32 -- fp32 operands, bit-equal
// to an fmaf chain -- so no scale, no split, and no range condition on h0 or the weights:
//   wave w owns units 32 w .. 32 w + 31 as two row blocks; lane (col = lane & 15, quad = lane >> 4) holds gates i, f, g, o of
//   units 32 w + 16 rb + 4 quad + r of sequence col: 8 accumulators of 16 x 16, started at the fp32 pre-activations.
//   W_hh in fp32 is the size of the two fp16 planes (1 MiB per direction at H = 256) and is streamed the same way: the host
//   packs it into fragment order -- per (wave, k-group of 16, row block, gate) 64 lanes x 16 bytes, lane (row = lane & 15, kq =
//   lane >> 4) holding W[row][16 kg + 4 kq + e], e = 0 .. 3: the A operands of four consecutive MFMAs -- and every wave reads
//   its slice as 1 KiB coalesced buffer loads at scalar offsets, a ring of (k-group, row block) sets ahead of the MFMAs.
//   h' crosses LDS as fp32 [buffer][sequence][k]: 16-byte writes (a lane's 4 units) and 16-byte reads (k = 16 kg + 4 quad + e,
//   the B operands of the same four MFMAs).  Every sum over k runs kg, then e, ascending, whatever the grid.
// The matrix pipe bounds the step: 16 x 4H x H MAC at 128 per clock and CU are 32.8 k cycles at H = 256.
// Pre-activations stay CHANNEL-MAJOR ([N][D*4H][ldt], ps_conv1x1_f32's layout: no transposition pass): 32 values per lane and
// step, fetched during the step before as 4-byte buffer loads -- one per-lane offset (the sequence's frame), the gate row as the
// scalar offset -- from a descriptor over the utterances the workgroup's 16 sequences span (the launcher keeps that below 2 GiB).
// Measured (profiles/lstm_h256_f32.txt): 21-24 us per step with few workgroups, 35-45 with consecutive-frame walks (every lane
// of such a load is a cache line of its own) -- not the 14-16 us of the matrix pipe alone; it beats the generic kernel
// from 128 sequences per launch on (H = 192: in two directions only), where the Python dispatch takes it (hip.H256_F32_MIN_SEQS).
// Only frames of real steps of real sequences are read: steps past the end re-read the last one, lanes past the last sequence
// replay it and store nothing.  The cell is lstm_kernel's (sigmoidf_, tanhf): the two differ in the order of the sums alone.
struct LstmH256F32 {
  ps_lstm_args a;
  const void* wimg;  // [D][H/32 waves][H/16 k-groups][2 row blocks][4 gates][64 lanes][4 floats]
  int span;          // utterances that 16 consecutive flat sequences can touch
};

template <int H>
__global__ __launch_bounds__(2 * H, 1) void lstm_h256_f32_kernel(LstmH256F32 k) {
  static_assert(H % 32 == 0 && H <= 256, "32 units per wave, at most 8 waves");
  constexpr int G = 4 * H, LDK = H + 4, NW = H / 32, NIT = H / 8;  // NIT: (k-group, row block) iterations per step
  __shared__ __attribute__((aligned(16))) float hb[2][16][LDK];
  const ps_lstm_args& a = k.a;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, quad = lane >> 4;
  const int d = blockIdx.z;
  const bool rev = d == 1;
  const int steps = a.steps;
  const int b0 = blockIdx.x * 16;
  const int b = b0 + col;
  const int seqs = a.N * a.Q;
  const bool valid = b < seqs;
  const int bb = valid ? b : seqs - 1;  // (lanes past the end replay the last sequence; nothing of theirs is stored)
  const int n = bb / a.Q, q = bb % a.Q;

  float c[2][4], h[2][4];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int r = 0; r < 4; ++r) c[rb][r] = 0.f, h[rb][r] = 0.f;
  if (valid && (a.h0 || a.c0)) {
    const int bs = b - a.state_shift;
    if (bs >= 0) {
      const int nn = bs / a.Q, qq = bs % a.Q;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t off = ((size_t)(nn * a.D + d) * H + 32 * w + 16 * rb + 4 * quad + r) * a.ldq + qq;
          if (a.h0) h[rb][r] = a.h0[off];
          if (a.c0) c[rb][r] = a.c0[off];
        }
    }
  }
  auto put_h = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
      *reinterpret_cast<f32x4*>(&hb[buf][col][32 * w + 16 * rb + 4 * quad]) = f32x4{h[rb][0], h[rb][1], h[rb][2], h[rb][3]};
  };
  put_h(0);

  // pre-activations: the descriptor starts at gate row (d, 32 w) of the group's first utterance and ends with its last one
  const int n0 = b0 / a.Q;
  const size_t slab = (size_t)a.D * G * a.ldt;  // floats per utterance
  const size_t row0 = (size_t)(d * G + 32 * w) * a.ldt;
  const int nspan = a.N - n0 < k.span ? a.N - n0 : k.span;
  const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.gx) + (size_t)n0 * slab + row0, 0, (int)(((size_t)nspan * slab - row0) * sizeof(float)), 0x00020000);
  const unsigned glane = (unsigned)(((size_t)(n - n0) * slab + (size_t)(4 * quad) * a.ldt + (size_t)q * a.q_stride) * sizeof(float));
  const unsigned rowb = (unsigned)a.ldt * (unsigned)sizeof(float);
  // the NEXT step's pre-activations [row block][gate][r].  Loads return in order, so a fragment load issued behind a burst of 32
  // scattered 4-byte loads waits for all of them: they leave two or three per iteration over the first half of the step instead
  float pre[2][4][4];
  auto pre_offset = [&](int s) __attribute__((always_inline)) {
    const int sc = s < steps ? s : steps - 1;
    const int ts = rev ? steps - 1 - sc : sc;
    return glane + (unsigned)ts * (unsigned)a.step_stride * (unsigned)sizeof(float);
  };
  auto load_pre = [&](int idx, unsigned vo) __attribute__((always_inline)) {
    const int rb = idx >> 4, g = (idx >> 2) & 3, r = idx & 3;
    pre[rb][g][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(gr, vo, (g * H + 16 * rb + r) * rowb, 0));
  };
  {
    const unsigned vo = pre_offset(0);
#pragma unroll
    for (int idx = 0; idx < 32; ++idx) load_pre(idx, vo);
  }

  // weight fragments of iteration it = 2 kg + rb: gate g at it * 4 + g (1 KiB units) of the wave's slice
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(k.wimg)) + (size_t)(d * NW + w) * NIT * 4096, 0, NIT * 4096,
      0x00020000);
  const int wlane = lane * 16;
  auto load_a = [&](int it, int g) __attribute__((always_inline)) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, wlane, (it * 4 + g) * 1024, 0));
  };
  float* hp = a.hout + ((size_t)(n * a.D + d) * H + 32 * w + 4 * quad) * a.ldt + (size_t)q * a.q_stride;
  __syncthreads();

  // a ring of RING (k-group, row block) fragment sets, PD of them in flight
  constexpr int RING = 4, PD = 3;
  static_assert(NIT % RING == 0, "the ring index of an iteration is the same in every step");
  f32x4 A[RING][4];
#pragma unroll
  for (int it = 0; it < PD; ++it)
#pragma unroll
    for (int g = 0; g < 4; ++g) A[it][g] = load_a(it, g);
  int buf = 0;
  size_t hoff = 0;  // frame offset of the step whose h' is still to be stored
  for (int s = 0; s < steps; ++s) {
    f32x4 acc[2][4];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[rb][g] = f32x4{pre[rb][g][0], pre[rb][g][1], pre[rb][g][2], pre[rb][g][3]};
    const unsigned vo = pre_offset(s + 1);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int kg = it >> 1, rb = it & 1;
      // the fragments of iteration it + PD (of the NEXT step past the end: the image does not depend on the step) leave now
#pragma unroll
      for (int g = 0; g < 4; ++g) A[(it + PD) % RING][g] = load_a((it + PD) % NIT, g);
      if (it < NIT / 2) {
#pragma unroll
        for (int idx = it * 32 / (NIT / 2); idx < (it + 1) * 32 / (NIT / 2); ++idx) load_pre(idx, vo);
      } else if (it < NIT / 2 + 8) {  // ... and the PREVIOUS step's h' behind them, one store per iteration
        const int idx = it - NIT / 2;
        if (s > 0 && valid) hp[(size_t)(16 * (idx >> 2) + (idx & 3)) * a.ldt + hoff] = h[idx >> 2][idx & 3];
      }
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&hb[buf][col][16 * kg + 4 * quad]);
      // four gates = four independent accumulators between two MFMAs on the same one (40 cycles dependent, 32 to issue)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[rb][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[it % RING][g][e], bv[e], acc[rb][g], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);  // (keeps the scheduler from hoisting several iterations' fragment loads)
    }
    hoff = (size_t)(rev ? steps - 1 - s : s) * a.step_stride;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gi = sigmoidf_(acc[rb][0][r]);
        const float gf = sigmoidf_(acc[rb][1][r]);
        const float gg = tanhf(acc[rb][2][r]);
        const float go = sigmoidf_(acc[rb][3][r]);
        c[rb][r] = gf * c[rb][r] + gi * gg;
        h[rb][r] = go * tanhf(c[rb][r]);
      }
    put_h(buf ^ 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (h' is in LDS; the stores and the prefetched loads stay in flight)
    __builtin_amdgcn_s_barrier();
    buf ^= 1;
  }
  if (valid) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) hp[(size_t)(16 * rb + r) * a.ldt + hoff] = h[rb][r];  // the last step's h'
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t off = ((size_t)(n * a.D + d) * H + 32 * w + 16 * rb + 4 * quad + r) * a.ldq + q;
        if (a.h_last) a.h_last[off] = h[rb][r];
        if (a.c_last) a.c_last[off] = c[rb][r];
      }
  }
}
