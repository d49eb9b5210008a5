// Stand-ins for what the Conv-TasNet masker driver (puresound_amd/csrc/abi.hip) calls, for test_masker_driver_calls.py:
// every launching entry appends one line to a ledger and returns 0 (ps_conv1x1_bf16_io first refuses a plane count that is
// neither 1 nor 3, as the real one does); the five pure answers are laws the test can override.
// Pointers are printed as symbols resolved against the ranges the test registers, so a ledger holds no address.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "puresound_hip.h"

namespace ps {
void set_error(const char* fmt, ...);  // abi.hip's
}

namespace {

struct Symbol {
  std::string name;
  const char* base;
  size_t bytes;  // 1: the pointer itself; more: a range, printed as name+OFFSET
};
std::vector<Symbol> g_symbols;
std::string g_ledger;
int g_absmax_parts = 64, g_dwconv_amax_ok = -1, g_f16_rows_ok = 0;
bool g_recording = true;  // off: the entries return at once (for timing the driver's own host work)

std::string sym(const void* p) {
  if (!p) return "null";
  for (const Symbol& s : g_symbols) {
    const char* c = (const char*)p;
    if (c < s.base || c >= s.base + s.bytes) continue;
    return s.bytes == 1 ? s.name : s.name + "+" + std::to_string((size_t)(c - s.base));
  }
  char buf[32];
  snprintf(buf, sizeof(buf), "?%p", p);
  return buf;
}

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}

std::string pro_text(const ps_prologue* p) {
  if (!p) return "pro=null";
  return fmt("pro={norm=%d prelu=%d stats=%s parts=%d count=%.17g eps=%.9g gamma=%s beta=%s slope=%s pre_relu=%d post_tanh=%d}",
             p->norm, p->prelu, sym(p->stats).c_str(), p->parts, p->count, p->eps, sym(p->gamma).c_str(),
             sym(p->beta).c_str(), sym(p->slope).c_str(), p->pre_relu, p->post_tanh);
}

std::string rng_text(const ps_f16x2_range* r) {
  if (!r) return "rng=null";
  return fmt("rng={w_exp=%d x_bound=%.9g x_amax=%s x_amax_parts=%d y_amax=%s amax_mul=%.9g amax_add=%.9g}", r->w_exp,
             r->x_bound, sym(r->x_amax).c_str(), r->x_amax_parts, sym(r->y_amax).c_str(), r->amax_mul, r->amax_add);
}

// what every GEMM entry shares behind its operands
std::string gemm_tail(int N, int K, int M, int T, int ldt, const ps_prologue* pro, const void* bias, const void* bias_n,
                      const void* res, const void* ostats, const void* stream) {
  return fmt("N=%d K=%d M=%d T=%d ldt=%d %s bias=%s bias_n=%s res=%s ostats=%s stream=%s", N, K, M, T, ldt,
             pro_text(pro).c_str(), sym(bias).c_str(), sym(bias_n).c_str(), sym(res).c_str(), sym(ostats).c_str(),
             sym(stream).c_str());
}

std::string dw_tail(int N, int H, int T, int ldt, int P, int dilation, int left, const ps_prologue* pro) {
  return fmt("N=%d H=%d T=%d ldt=%d P=%d dilation=%d left=%d %s", N, H, T, ldt, P, dilation, left, pro_text(pro).c_str());
}

int record(const std::string& line) {
  g_ledger += line;
  g_ledger += '\n';
  return 0;
}

}  // namespace

extern "C" {

void probe_register(const char* name, const void* base, size_t bytes) { g_symbols.push_back({name, (const char*)base, bytes}); }
void probe_forget(void) { g_symbols.clear(); }
void probe_clear(void) { g_ledger.clear(); }
const char* probe_ledger(void) { return g_ledger.c_str(); }
void probe_recording(int on) { g_recording = on != 0; }
// absmax_parts: the answer; dwconv_amax_ok: 0 / 1, or -1 for the library's law (P = 3, 2 * dilation <= 256); f16_rows_ok: 0 / 1
void probe_answers(int absmax_parts, int dwconv_amax_ok, int f16_rows_ok) {
  g_absmax_parts = absmax_parts;
  g_dwconv_amax_ok = dwconv_amax_ok;
  g_f16_rows_ok = f16_rows_ok;
}

// two laws that differ from each other at the same (channels, frames) and between C = 8 and H = 4
int ps_conv1x1_stats_parts(int M, int T) { return M <= 0 || T <= 0 ? 0 : 2 * M + (T + 31) / 32; }
int ps_dwconv_stats_parts(int H, int T) { return H <= 0 || T <= 0 ? 0 : 3 * H + (T + 63) / 64 + 1; }
int ps_absmax_parts(void) { return g_absmax_parts; }
int ps_dwconv_amax_ok(int P, int dilation, int left) {
  return g_dwconv_amax_ok >= 0 ? g_dwconv_amax_ok : (P == 3 && 2 * dilation <= 256 && left >= 0 && left <= 2 * dilation);
}
int ps_conv1x1_f16_rows_ok(int N, int K, int M, int T) { return N > 0 && K > 0 && M > 0 && T > 0 ? g_f16_rows_ok : 0; }

int ps_embed_bias_f32(const float* dvec, const float* w_embed, float* bias_n, int N, int E, int M, int normalize,
                      void* stream) {
  if (!g_recording) return 0;
  return record(fmt("ps_embed_bias_f32 dvec=%s w_embed=%s bias_n=%s N=%d E=%d M=%d normalize=%d stream=%s", sym(dvec).c_str(),
                    sym(w_embed).c_str(), sym(bias_n).c_str(), N, E, M, normalize, sym(stream).c_str()));
}

int ps_conv1x1_f32(const float* x, const float* wt, float* y, int N, int K, int M, int T, int ldt, const ps_prologue* pro,
                   const float* bias, const float* bias_n, const float* res, double* ostats, void* stream) {
  if (!g_recording) return 0;
  return record(fmt("ps_conv1x1_f32 x=%s wt=%s y=%s ", sym(x).c_str(), sym(wt).c_str(), sym(y).c_str()) +
                gemm_tail(N, K, M, T, ldt, pro, bias, bias_n, res, ostats, stream));
}

int ps_conv1x1_f16x2_f32(const float* x, const void* wt_planes, const ps_f16x2_range* rng, float* y, int N, int K, int M,
                         int T, int ldt, const ps_prologue* pro, const float* bias, const float* bias_n, const float* res,
                         double* ostats, void* stream) {
  if (!g_recording) return 0;
  return record(fmt("ps_conv1x1_f16x2_f32 x=%s wt_planes=%s %s y=%s ", sym(x).c_str(), sym(wt_planes).c_str(),
                    rng_text(rng).c_str(), sym(y).c_str()) +
                gemm_tail(N, K, M, T, ldt, pro, bias, bias_n, res, ostats, stream));
}

int ps_conv1x1_f16_rows(const void* x, const void* wt_planes, const ps_f16x2_range* rng, void* y, int N, int K, int M, int T,
                        int ldt, const ps_prologue* pro, const float* bias, const float* bias_n, const void* res,
                        double* ostats, void* stream) {
  if (!g_recording) return 0;
  return record(fmt("ps_conv1x1_f16_rows x=%s wt_planes=%s %s y=%s ", sym(x).c_str(), sym(wt_planes).c_str(),
                    rng_text(rng).c_str(), sym(y).c_str()) +
                gemm_tail(N, K, M, T, ldt, pro, bias, bias_n, res, ostats, stream));
}

int ps_conv1x1_bf16_io(const void* x, int x_bf16, const void* wt_planes, void* y, int y_bf16, int N, int K, int M, int T,
                       int ldt, int planes, const ps_prologue* pro, const float* bias, const float* bias_n, const float* res,
                       double* ostats, void* stream) {
  if (planes != 1 && planes != 3) {  // the one refusal of an entry that the driver relied on: the entry's own words
    ps::set_error("ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got %d", planes);
    return PS_E_INVALID;
  }
  if (!g_recording) return 0;
  return record(fmt("ps_conv1x1_bf16_io x=%s x_bf16=%d wt_planes=%s y=%s y_bf16=%d planes=%d ", sym(x).c_str(), x_bf16,
                    sym(wt_planes).c_str(), sym(y).c_str(), y_bf16, planes) +
                gemm_tail(N, K, M, T, ldt, pro, bias, bias_n, res, ostats, stream));
}

int ps_dwconv_io(const void* x, int x_bf16, const float* w, const float* b, void* y, int y_bf16, int N, int H, int T, int ldt,
                 int P, int dilation, int left, const ps_prologue* pro, double* ostats, void* stream) {
  if (!g_recording) return 0;
  return record(fmt("ps_dwconv_io x=%s x_bf16=%d w=%s b=%s y=%s y_bf16=%d ", sym(x).c_str(), x_bf16, sym(w).c_str(),
                    sym(b).c_str(), sym(y).c_str(), y_bf16) +
                dw_tail(N, H, T, ldt, P, dilation, left, pro) +
                fmt(" ostats=%s stream=%s", sym(ostats).c_str(), sym(stream).c_str()));
}

int ps_dwconv_amax_f32(const float* x, const float* w, const float* b, float* y, int N, int H, int T, int ldt, int P,
                       int dilation, int left, const ps_prologue* pro, float* y_amax, void* stream) {
  if (!g_recording) return 0;
  return record(fmt("ps_dwconv_amax_f32 x=%s w=%s b=%s y=%s ", sym(x).c_str(), sym(w).c_str(), sym(b).c_str(), sym(y).c_str()) +
                dw_tail(N, H, T, ldt, P, dilation, left, pro) +
                fmt(" y_amax=%s stream=%s", sym(y_amax).c_str(), sym(stream).c_str()));
}

int ps_absmax_f32(const float* x, float* amax, int N, int C, int T, int ldt, void* stream) {
  if (!g_recording) return 0;
  return record(fmt("ps_absmax_f32 x=%s amax=%s N=%d C=%d T=%d ldt=%d stream=%s", sym(x).c_str(), sym(amax).c_str(), N, C, T,
                    ldt, sym(stream).c_str()));
}

}  // extern "C"
