// C-ABI glue: error reporting, sizing helpers and the network-level drivers that enqueue one TCN block
// (conv_tasnet.py:67-90 of mcw519/PureSound) and the whole Conv-TasNet masker (conv_tasnet.py:338-359).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include <atomic>

#include "ps_common.h"

namespace ps {

static thread_local char g_err[512] = "";
int g_debug_flags = 0;
int g_debug_grid_cap = 0;
int g_debug_ablate = 0;
void* g_debug_buffer = nullptr;

static void vset_error(const char* fmt, va_list ap) { vsnprintf(g_err, sizeof(g_err), fmt, ap); }

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vset_error(fmt, ap);
  va_end(ap);
}

int launch_status(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

int check_prologue(const char* who, const ps_prologue* pro) {
  if (!pro) return 0;
  if (pro->norm == PS_NORM_GLOBAL && (!pro->stats || pro->parts <= 0 || pro->count <= 0 || !pro->gamma || !pro->beta)) {
    set_error("%s: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta", who);
    return PS_E_INVALID;
  }
  if (pro->norm == PS_NORM_AFFINE && (!pro->gamma || !pro->beta)) {
    set_error("%s: PS_NORM_AFFINE prologue needs gamma/beta", who);
    return PS_E_INVALID;
  }
  if (pro->prelu && !pro->slope) {
    set_error("%s: prelu prologue needs slope", who);
    return PS_E_INVALID;
  }
  return 0;
}

struct ProfRecord {
  const char* kernel;
  hipEvent_t start, stop;
};
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfRecord> g_prof;

LaunchTimer::LaunchTimer(const char* kernel, hipStream_t stream) : slot_(-1), stream_(stream) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRecord r{kernel, nullptr, nullptr};
  if (hipEventCreate(&r.start) != hipSuccess || hipEventCreate(&r.stop) != hipSuccess) return;
  (void)hipEventRecord(r.start, stream);
  g_prof.push_back(r);
  slot_ = (int)g_prof.size() - 1;
}

LaunchTimer::~LaunchTimer() {
  if (slot_ < 0) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  (void)hipEventRecord(g_prof[slot_].stop, stream_);
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace ps

using namespace ps;

namespace ps {
int device_cus() {
  static std::atomic<int> cache[64];  // 0 = not read yet
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  int cus = cache[dev].load(std::memory_order_relaxed);
  if (cus == 0) {
    hipDeviceProp_t prop;
    cus = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 0;
    if (cus <= 0) cus = 256;
    cache[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}
}  // namespace ps

extern "C" int ps_abi_version(void) { return PS_ABI_VERSION; }
extern "C" const char* ps_last_error(void) { return g_err; }

static int swap_if_set(int& g, int v) {
  const int old = g;
  if (v >= 0) g = v;
  return old;
}
extern "C" int ps_debug_flags(int flags) { return swap_if_set(g_debug_flags, flags); }
extern "C" int ps_debug_grid_cap(int cap) { return swap_if_set(g_debug_grid_cap, cap); }
extern "C" int ps_debug_ablate(int mask) { return swap_if_set(g_debug_ablate, mask); }

extern "C" int ps_debug_buffer(void* device_buffer) {
  g_debug_buffer = device_buffer;
  return 0;
}

extern "C" int ps_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (on) {
    for (auto& r : g_prof) {
      (void)hipEventDestroy(r.start);
      (void)hipEventDestroy(r.stop);
    }
    g_prof.clear();
  }
  g_prof_on = on != 0;
  return 0;
}

extern "C" int ps_profile_read(const char* kernel, double* total_ms, int* launches) {
  if (!kernel || !total_ms || !launches) {
    set_error("ps_profile_read: null argument");
    return PS_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double tot = 0.0;
  int cnt = 0;
  for (auto& r : g_prof) {
    if (strcmp(r.kernel, kernel) != 0) continue;
    hipError_t e = hipEventSynchronize(r.stop);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, r.start, r.stop);
    if (e != hipSuccess) {
      set_error("ps_profile_read: %s", hipGetErrorString(e));
      return (int)e;
    }
    tot += ms;
    ++cnt;
  }
  *total_ms = tot;
  *launches = cnt;
  return 0;
}

// Rows are padded to an ODD multiple of 128 frames (512 B): a power-of-two row stride (T=3999 -> 16 KiB)
// would put the same column of every channel row on the same HBM channels ("channel camping").
extern "C" int ps_padded_frames(int frames) {
  if (frames <= 0) return 0;
  int tiles = ceil_div(frames, kTileT);
  if ((tiles & 1) == 0) ++tiles;
  return tiles * kTileT;
}

extern "C" int ps_stats_parts(int channels, int frames) {
  if (channels <= 0 || frames <= 0) return 0;
  const int gemm = ps_conv1x1_stats_parts(channels, frames);
  const int dw = ps_dwconv_stats_parts(channels, frames);
  return gemm > dw ? gemm : dw;
}

// Workspace carve-up for ps_conv_tasnet_f32 (TasnetWs, ps_common.h)
namespace ps {
TasnetWs carve(void* base, int N, int C, int H, int T) {
  TasnetWs w{};
  const int ldt = ps_padded_frames(T);
  // parts must cover producers with up to max(C,H) channels; H is what every stats producer emits
  w.parts = ps_stats_parts(H, T);
  const size_t map = align_up((size_t)N * H * ldt * sizeof(float), 256);
  const size_t st = align_up((size_t)N * w.parts * 2 * sizeof(double), 256);
  const size_t bn = align_up((size_t)N * H * sizeof(float), 256);
  w.amax_parts = ps_conv1x1_stats_parts(C > 0 ? C : H, T);
  if (w.amax_parts < ps_absmax_parts()) w.amax_parts = ps_absmax_parts();
  const size_t am = align_up((size_t)N * w.amax_parts * sizeof(float), 256);
  char* p = (char*)base;
  w.y1 = (float*)p; p += map;
  w.y2 = (float*)p; p += map;
  w.y3 = (float*)p; p += map;
  w.s1 = (double*)p; p += st;
  w.s2 = (double*)p; p += st;
  w.s3 = (double*)p; p += st;
  w.bias_n = (float*)p; p += bn;
  w.amax[0] = (float*)p; p += am;
  w.amax[1] = (float*)p; p += am;
  w.bytes = (size_t)(p - (char*)base);
  return w;
}
}  // namespace ps

extern "C" size_t ps_conv_tasnet_workspace_bytes(int N, int C, int H, int T) {
  if (N <= 0 || C <= 0 || H <= 0 || T <= 0) return 0;
  return carve(nullptr, N, C, H, T).bytes;
}

// The driver: helpers, the checks, the per-block plan, the launch path, the three entries.
namespace ps {
int dw_left(int P, int dilation, int causal) { return causal ? (P - 1) * dilation : ((P - 1) / 2) * dilation; }
}  // namespace ps

// gemm_planes = 2 behind a folded BatchNorm (bN1d blocks: no bound on the normalised values exists): the producer leaves the
// maxima of its output behind -- in the statistics slots such a norm has no use for -- and the consumer maps them through the
// norm's largest scale and shift
static bool measured_behind(const ps_tcn_block& b, int norm) { return b.gemm_planes == 2 && norm == PS_NORM_AFFINE; }

// the maxima of the depthwise output come from the kernel that measures while it writes, or from one ps_absmax_f32 pass
// into a statistics slot of ws_parts (sum, sum of squares) pairs
static bool dw_maxima_have_room(int P, int dilation, int causal, int ws_parts) {
  return ps_dwconv_amax_ok(P, dilation, dw_left(P, dilation, causal)) ||
         (size_t)ps_absmax_parts() * sizeof(float) <= (size_t)ws_parts * 2 * sizeof(double);
}

// bf16 rows (sb): launches the register-B kernel takes run with ONE fp16 product per multiply-add (ps_conv1x1_f16_rows)
// whenever the block carries the fp16 weight image and the input's range is known; behind a norm that is a global one
static bool out_conv_on_f16_rows(const ps_tcn_block& b, int sb, int N, int T) {
  return sb && b.out_wf && b.pw_norm == PS_NORM_GLOBAL && ps_conv1x1_f16_rows_ok(N, b.H, b.C, T);
}

// THE rule for the range chain: this block's out_conv leaves the partial maxima of the stream for the next in_conv, and its
// own in_conv reads those the block before left -- fp16x2 blocks, and bf16-rows blocks on the f16-rows kernel at both ends
static bool leaves_maxima(const ps_tcn_block& b, int sb, int N, int T) {
  return b.gemm_planes == 2 || (out_conv_on_f16_rows(b, sb, N, T) && b.in_wf);
}

// norm + PReLU in front of a consumer: GlobLN.eps and gGN's eps (lobe/norm.py:10,96); a folded BN carries its own
namespace ps {
ps_prologue norm_prelu(int norm, const double* stats, int parts, double count, const float* gamma, const float* beta,
                       const float* slope) {
  return ps_prologue{norm, /*prelu*/ 1, stats, parts, count, /*eps*/ 1e-8f, gamma, beta, slope, /*pre_relu*/ 0, /*post_tanh*/ 0};
}
}  // namespace ps

// The range descriptor of GEMM `which` (0 / 1 / 2: in_conv, pointwise, out_conv) in the fp16x2 and the f16-rows arithmetic.
// in_conv: the maxima of the stream (x_amax).  Behind a norm (gmax / bmax: its largest scale and shift, times
// max(1, |slope|), from the planner): the producer's measured maxima when there are any, else the bound of a global norm.
static ps_f16x2_range gemm_range(const ps_tcn_block& b, int which, double count, const float* x_amax, int x_amax_parts,
                                 float* y_amax) {
  ps_f16x2_range rng{};
  rng.w_exp = b.w_exp[which], rng.y_amax = y_amax;
  const float gmax = which == 1 ? b.dw_gmax : b.pw_gmax, bmax = which == 1 ? b.dw_bmax : b.pw_bmax;
  if (which == 0 || (x_amax && gmax > 0.f)) {
    rng.x_amax = x_amax;
    rng.x_amax_parts = x_amax_parts;
    // behind a per-channel affine map: |scale_c v + shift_c| <= max|scale| max|v| + max|shift|
    rng.amax_mul = which == 0 ? 0.f : gmax;
    rng.amax_add = which == 0 ? 0.f : bmax;
  } else if (x_amax) {
    rng.x_bound = bmax > 0.f ? bmax : 1.f;  // (scale = 0: the map is the constant shift)
  } else {
    // behind a global norm |z| <= sqrt(count - 1), so |gamma z + beta| <= max|gamma| sqrt(count) + max|beta|
    rng.x_bound = gmax * (float)sqrt(count) + bmax;
    if (!(rng.x_bound > 0.f)) rng.x_bound = 1.f;  // (gamma = beta = 0: every value is 0)
  }
  return rng;
}

// sets the message and hands back the code
static int refuse(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vset_error(fmt, ap);
  va_end(ap);
  return code;
}

// The rules of the arguments and of the blocks' sizes that every masker driver shares (ragged.hip's too), in the order the
// entries have always given them
namespace ps {
int check_stack(const ps_tcn_block* blocks, int n_blocks, const float* x_in, const float* x_out, int N, int T, int ldt,
                const void* workspace, size_t workspace_bytes) {
  if (!blocks || n_blocks <= 0 || !x_in || !x_out || !workspace || N <= 0 || T <= 0)
    return refuse(PS_E_INVALID, "ps_conv_tasnet_f32: null pointer or non-positive size");
  if (x_in == x_out)
    return refuse(PS_E_INVALID, "ps_conv_tasnet_f32: x_in must not alias x_out (the input is never modified)");
  if (ldt != ps_padded_frames(T))
    return refuse(PS_E_ALIGN, "ps_conv_tasnet_f32: ldt=%d must be ps_padded_frames(T=%d)=%d", ldt, T, ps_padded_frames(T));
  const int C = blocks[0].C, H = blocks[0].H;
  for (int i = 0; i < n_blocks; ++i) {
    const ps_tcn_block& b = blocks[i];
    if (b.C != C || b.H != H || b.P <= 0 || b.dilation <= 0)
      return refuse(PS_E_INVALID, "ps_conv_tasnet_f32: block %d has inconsistent sizes (C=%d H=%d P=%d dilation=%d)", i, b.C,
                    b.H, b.P, b.dilation);
    // reference: AssertionError in DepthwiseSeparableConv1d (lobe/cnn.py:40-44)
    if (b.causal && (b.in_norm == PS_NORM_GLOBAL || b.dw_norm == PS_NORM_GLOBAL || b.pw_norm == PS_NORM_GLOBAL))
      return refuse(PS_E_INVALID, "ps_conv_tasnet_f32: block %d: global norms conflict with causal=1", i);
  }
  const size_t need = ps_conv_tasnet_workspace_bytes(N, C, H, T);
  if (workspace_bytes < need)
    return refuse(PS_E_INVALID, "ps_conv_tasnet_f32: workspace too small (%zu < %zu)", workspace_bytes, need);
  if ((uintptr_t)workspace & 255) return refuse(PS_E_ALIGN, "ps_conv_tasnet_f32: workspace must be 256-byte aligned");
  return 0;
}
}  // namespace ps

// Everything a call can be refused for, before the first launch: the arguments, then block by block
static int check_call(const ps_tcn_block* blocks, int n_blocks, const float* x_in, float* x_out, const float* dvec,
                      int embed_norm, int N, int T, int ldt, void* workspace, size_t workspace_bytes, const float* x_amax,
                      int x_amax_parts, void* stream, int sb) {
  if (x_amax && x_amax_parts <= 0) return refuse(PS_E_INVALID, "ps_conv_tasnet_ranged_f32: x_amax needs x_amax_parts > 0");
  if (const int rc = check_stack(blocks, n_blocks, x_in, x_out, N, T, ldt, workspace, workspace_bytes)) return rc;
  const int H = blocks[0].H;
  const int ws_parts = ps_stats_parts(H, T);
  const auto ranged = [](int norm) { return norm == PS_NORM_GLOBAL || norm == PS_NORM_AFFINE; };
  for (int i = 0; i < n_blocks; ++i) {
    const ps_tcn_block& b = blocks[i];
    if (sb && (b.gemm_planes != 1 || !b.hidden_bf16))
      return refuse(PS_E_UNSUPPORTED,
                    "ps_conv_tasnet_bf16_rows: block %d is not in the bf16 arithmetic (gemm_planes = 1, hidden_bf16)", i);
    if (b.in_embed_w && !dvec)
      return refuse(PS_E_INVALID, "ps_conv_tasnet_f32: block expects an embedding (E=%d) but dvec is NULL", b.E);
    // (the range of the block's input is never missing: the caller's, the block before's, or one ps_absmax_f32 pass, whose
    // ps_absmax_parts() is a positive constant)
    if (b.gemm_planes == 2 && (!ranged(b.dw_norm) || !ranged(b.pw_norm)))
      return refuse(PS_E_UNSUPPORTED,
                    "ps_conv_tasnet_f32: gemm_planes=2 (fp16x2) needs a global norm (a bound on the normalised values) or a "
                    "per-channel affine norm (the producer's measured maxima) in front of the pointwise and output convs, and "
                    "the range of the block's input");
    if (b.gemm_planes != 0 && (!b.in_wb || !b.pw_wb || !b.out_wb))
      return refuse(PS_E_INVALID, "ps_conv_tasnet_f32: gemm_planes=%d needs the plane-packed weights in_wb / pw_wb / out_wb",
                    b.gemm_planes);
    if (b.gemm_planes < 0 || b.gemm_planes > 3)  // (what ps_conv1x1_bf16_io would answer at the block's first GEMM)
      return refuse(PS_E_INVALID, "ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got %d",
                    b.gemm_planes);
    if (measured_behind(b, b.dw_norm) && !dw_maxima_have_room(b.P, b.dilation, b.causal, ws_parts))
      return refuse(PS_E_UNSUPPORTED, "ps_conv_tasnet_f32: no room for the maxima of the depthwise output (T=%d)", T);
  }
  return 0;
}

// What one block enqueues, decided without launching.  The three GEMMs (0 / 1 / 2: in_conv, pointwise, out_conv) each run
// on one of five entries: exact fp32 MFMA; fp16x2; bf16 rows with one fp16 product; the bf16 pipe with 1 / 3 operand planes.
// hidden_bf16 (with gemm_planes = 1): y1, y2, y3 -- which never leave the workspace -- are bf16 rows.
enum GemmEntry { GEMM_F32, GEMM_F16X2, GEMM_F16_ROWS, GEMM_BF16_PLANES_1, GEMM_BF16_PLANES_3 };
enum DwEntry { DW_MEASURING, DW_IO, DW_IO_THEN_ABSMAX };  // (the last: a shape outside the kernel that measures while it writes)
struct BlockPlan {
  GemmEntry gemm[3];
  ps_f16x2_range rng[3];  // GEMM_F16X2 and GEMM_F16_ROWS
  DwEntry dw;
  int hb;        // the hidden maps are bf16 rows
  float *a2, *a3;  // where the maxima of y2 / y3 go (fp16x2 behind a folded BatchNorm), else NULL
};

// x_amax / x_amax_parts: partial maxima of the block's input, or NULL; y_amax: where out_conv leaves those of x_out, or NULL
static BlockPlan plan_block(const ps_tcn_block& b, int N, int T, const TasnetWs& w, int sb, const float* x_amax,
                            int x_amax_parts, float* y_amax) {
  BlockPlan p{};
  const double count = (double)b.H * (double)T;
  p.hb = (b.hidden_bf16 && b.gemm_planes == 1) ? 1 : 0;
  p.a2 = measured_behind(b, b.dw_norm) ? reinterpret_cast<float*>(w.s2) : nullptr;
  p.a3 = measured_behind(b, b.pw_norm) ? reinterpret_cast<float*>(w.s3) : nullptr;
  p.dw = !p.a2 ? DW_IO : ps_dwconv_amax_ok(b.P, b.dilation, dw_left(b.P, b.dilation, b.causal)) ? DW_MEASURING : DW_IO_THEN_ABSMAX;
  const int a2_parts = p.dw == DW_MEASURING ? ps_dwconv_stats_parts(b.H, T) : ps_absmax_parts();
  const GemmEntry plain = b.gemm_planes == 0 ? GEMM_F32 : b.gemm_planes == 2 ? GEMM_F16X2  // (check_call: 0 .. 3)
                          : b.gemm_planes == 1 ? GEMM_BF16_PLANES_1 : GEMM_BF16_PLANES_3;
  p.gemm[0] = p.gemm[1] = p.gemm[2] = plain;
  if (sb) {
    if (b.in_wf && x_amax && ps_conv1x1_f16_rows_ok(N, b.C, b.H, T)) p.gemm[0] = GEMM_F16_ROWS;
    if (b.pw_wf && b.dw_norm == PS_NORM_GLOBAL && ps_conv1x1_f16_rows_ok(N, b.H, b.H, T)) p.gemm[1] = GEMM_F16_ROWS;
    if (out_conv_on_f16_rows(b, sb, N, T)) p.gemm[2] = GEMM_F16_ROWS;
  }
  p.rng[0] = gemm_range(b, 0, count, x_amax, x_amax_parts, nullptr);
  p.rng[1] = gemm_range(b, 1, count, p.a2, a2_parts, p.a3);
  p.rng[2] = gemm_range(b, 2, count, p.a3, ps_conv1x1_stats_parts(b.H, T), y_amax);
  return p;
}

// wt / wb / wf: the weight in kernel layout, plane-packed, and as the fp16 image of the f16-rows kernel
static int launch_gemm(GemmEntry entry, const ps_f16x2_range& rng, const float* x, int xb, const float* wt, const void* wb,
                       const void* wf, float* y, int yb, int N, int K, int M, int T, int ldt, const ps_prologue* pro,
                       const float* bias, const float* bn, const float* res, double* st, void* stream) {
  switch (entry) {
    case GEMM_F32: return ps_conv1x1_f32(x, wt, y, N, K, M, T, ldt, pro, bias, bn, res, st, stream);
    case GEMM_F16X2: return ps_conv1x1_f16x2_f32(x, wb, &rng, y, N, K, M, T, ldt, pro, bias, bn, res, st, stream);
    case GEMM_F16_ROWS: return ps_conv1x1_f16_rows(x, wf, &rng, y, N, K, M, T, ldt, pro, bias, bn, res, st, stream);
    case GEMM_BF16_PLANES_1: return ps_conv1x1_bf16_io(x, xb, wb, y, yb, N, K, M, T, ldt, 1, pro, bias, bn, res, st, stream);
    case GEMM_BF16_PLANES_3: return ps_conv1x1_bf16_io(x, xb, wb, y, yb, N, K, M, T, ldt, 3, pro, bias, bn, res, st, stream);
  }
  return PS_E_INVALID;
}

// sb: the residual stream (x_in, x_out) is bf16 rows too
static int launch_block(const ps_tcn_block& b, const BlockPlan& p, const float* x_in, float* x_out, const float* dvec,
                        int embed_norm, int N, int T, int ldt, const TasnetWs& w, void* stream, int sb) {
  int rc;
  const double count = (double)b.H * (double)T;
  const int gemm_parts_h = ps_conv1x1_stats_parts(b.H, T), dw_parts = ps_dwconv_stats_parts(b.H, T), hb = p.hb;

  // 1) in_conv (no bias) [+ per-utterance embedding bias]; stats of y1
  const float* bias_n = b.in_embed_w ? w.bias_n : nullptr;
  if (bias_n && (rc = ps_embed_bias_f32(dvec, b.in_embed_w, w.bias_n, N, b.E, b.H, embed_norm, stream))) return rc;
  rc = launch_gemm(p.gemm[0], p.rng[0], x_in, sb, b.in_wt, b.in_wb, b.in_wf, w.y1, hb, N, b.C, b.H, T, ldt, nullptr, nullptr,
                   bias_n, nullptr, b.in_norm == PS_NORM_GLOBAL ? w.s1 : nullptr, stream);
  if (rc) return rc;

  // 2) depthwise: prologue = in_conv's norm + PReLU; stats (or maxima) of y2
  const ps_prologue p1 = norm_prelu(b.in_norm, w.s1, gemm_parts_h, count, b.in_gamma, b.in_beta, b.in_slope);
  const int left = dw_left(b.P, b.dilation, b.causal);
  if (p.dw == DW_MEASURING) {
    rc = ps_dwconv_amax_f32(w.y1, b.dw_w, b.dw_b, w.y2, N, b.H, T, ldt, b.P, b.dilation, left, &p1, p.a2, stream);
  } else {
    rc = ps_dwconv_io(w.y1, hb, b.dw_w, b.dw_b, w.y2, hb, N, b.H, T, ldt, b.P, b.dilation, left, &p1,
                      b.dw_norm == PS_NORM_GLOBAL ? w.s2 : nullptr, stream);
    if (!rc && p.dw == DW_IO_THEN_ABSMAX) rc = ps_absmax_f32(w.y2, p.a2, N, b.H, T, ldt, stream);
  }
  if (rc) return rc;

  // 3) pointwise: prologue = depthwise norm + PReLU; stats of y3
  const ps_prologue p2 = norm_prelu(b.dw_norm, w.s2, dw_parts, count, b.dw_gamma, b.dw_beta, b.dw_slope);
  rc = launch_gemm(p.gemm[1], p.rng[1], w.y2, hb, b.pw_wt, b.pw_wb, b.pw_wf, w.y3, hb, N, b.H, b.H, T, ldt, &p2, b.pw_b,
                   nullptr, nullptr, b.pw_norm == PS_NORM_GLOBAL ? w.s3 : nullptr, stream);
  if (rc) return rc;

  // 4) out_conv + bias + residual: prologue = pointwise norm + PReLU
  const ps_prologue p3 = norm_prelu(b.pw_norm, w.s3, gemm_parts_h, count, b.pw_gamma, b.pw_beta, b.pw_slope);
  return launch_gemm(p.gemm[2], p.rng[2], w.y3, hb, b.out_wt, b.out_wb, b.out_wf, x_out, sb, N, b.H, b.C, T, ldt, &p3, b.out_b,
                     nullptr, x_in, nullptr, stream);
}

static int conv_tasnet_rows(const ps_tcn_block* blocks, int n_blocks, const float* x_in, float* x_out, const float* dvec,
                            int embed_norm, int N, int T, int ldt, void* workspace, size_t workspace_bytes,
                            const float* x_amax, int x_amax_parts, void* stream, int sb) {
  if (const int rc = check_call(blocks, n_blocks, x_in, x_out, dvec, embed_norm, N, T, ldt, workspace, workspace_bytes, x_amax,
                                x_amax_parts, stream, sb))
    return rc;
  const int C = blocks[0].C, H = blocks[0].H;
  const TasnetWs w = carve(workspace, N, C, H, T);
  // block 0 reads the caller's input and writes x_out; later blocks update x_out in place (each
  // workgroup reads exactly the residual elements it overwrites).
  int have_parts = 0;  // partial maxima of the current residual stream in w.amax[i & 1] (blocks that leave_maxima only)
  const int out_parts = ps_conv1x1_stats_parts(C, T);
  for (int i = 0; i < n_blocks; ++i) {
    const float* xi = i == 0 ? x_in : x_out;
    const bool f16 = leaves_maxima(blocks[i], sb, N, T);
    const float* range = w.amax[i & 1];
    if (f16 && i == 0 && x_amax) {  // the caller knows the range of x_in (maxima, or any upper bound per utterance)
      range = x_amax;
      have_parts = x_amax_parts;
    } else if (f16 && !have_parts && sb) {
      range = nullptr;  // (no pass over bf16 rows: this block's in_conv takes the planes = 1 kernel)
    } else if (f16 && !have_parts) {  // first fp16x2 block (or one behind another arithmetic): one pass over its input
      const int rc = ps_absmax_f32(xi, w.amax[i & 1], N, C, T, ldt, stream);
      if (rc) return rc;
      have_parts = ps_absmax_parts();
    }
    const BlockPlan plan = plan_block(blocks[i], N, T, w, sb, (f16 && have_parts) ? range : nullptr, have_parts,
                                      f16 ? w.amax[(i + 1) & 1] : nullptr);
    const int rc = launch_block(blocks[i], plan, xi, x_out, dvec, embed_norm, N, T, ldt, w, stream, sb);
    if (rc) return rc;
    have_parts = f16 ? out_parts : 0;
  }
  return 0;
}

extern "C" int ps_conv_tasnet_ranged_f32(const ps_tcn_block* blocks, int n_blocks, const float* x_in, float* x_out,
                                         const float* dvec, int embed_norm, int N, int T, int ldt, void* workspace,
                                         size_t workspace_bytes, const float* x_amax, int x_amax_parts, void* stream) {
  return conv_tasnet_rows(blocks, n_blocks, x_in, x_out, dvec, embed_norm, N, T, ldt, workspace, workspace_bytes, x_amax,
                          x_amax_parts, stream, 0);
}

extern "C" int ps_conv_tasnet_f32(const ps_tcn_block* blocks, int n_blocks, const float* x_in, float* x_out,
                                  const float* dvec, int embed_norm, int N, int T, int ldt, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return ps_conv_tasnet_ranged_f32(blocks, n_blocks, x_in, x_out, dvec, embed_norm, N, T, ldt, workspace, workspace_bytes,
                                   nullptr, 0, stream);
}

// BASELINE config 3's arithmetic ("bf16 storage / fp32 accumulate"): the residual stream is bf16 rows as well
extern "C" int ps_conv_tasnet_bf16_rows(const ps_tcn_block* blocks, int n_blocks, const void* x_in, void* x_out,
                                        const float* dvec, int embed_norm, int N, int T, int ldt, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return conv_tasnet_rows(blocks, n_blocks, (const float*)x_in, (float*)x_out, dvec, embed_norm, N, T, ldt, workspace,
                          workspace_bytes, nullptr, 0, stream, 1);
}
