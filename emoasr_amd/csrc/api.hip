// Library-level plumbing: error strings, version, run-time options.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include "common.h"
#include "../../include/emoasr_hip.h"

static thread_local char g_err[512] = "";

// see common.h
EmoScratch* emo_stream_scratch(int slot, void* stream, size_t bytes) {
  static std::mutex mu;
  static std::map<std::tuple<int, void*, int>, EmoScratch*> tab;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_tuple(dev, stream, slot);
  auto it = tab.find(key);
  if (it != tab.end() && it->second->bytes >= bytes) return it->second;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
    emo_set_error("stream scratch %d: first use on a stream that is being captured (run the call once eagerly on this stream)", slot);
    return nullptr;
  }
  void* d = nullptr;
  // cleared ON the stream that will use the area (ordered before its first launch there): a hipMemset on the null stream is not
  // ordered against a non-blocking stream, and a launch that started on a half-cleared barrier counter gave up waiting
  if (hipMalloc(&d, bytes) != hipSuccess || hipMemsetAsync(d, 0, bytes, (hipStream_t)stream) != hipSuccess) {
    emo_set_error("stream scratch %d: allocation of %zu bytes failed", slot, bytes);
    return nullptr;
  }
  EmoScratch* r = new EmoScratch{};   // (a grown area replaces the record; the old device area is leaked on purpose: launches may still use it)
  r->dev = d; r->bytes = bytes;
  tab[key] = r;
  return r;
}

void emo_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- run-time options: the list of common.h -------------------------------------------------------------------------------
EmoOptions g_opt = {
#define EMO_OPT_DEFAULT(name, def, norm, doc) def,
    EMO_OPTIONS(EMO_OPT_DEFAULT)
#undef EMO_OPT_DEFAULT
};
namespace {
struct OptionEntry { const char* name; int EmoOptions::*field; int def; int (*norm)(int); };
const OptionEntry kOptions[] = {
#define EMO_OPT_ENTRY(name, def, norm, doc) {#name, &EmoOptions::name, def, [](int v) -> int { return norm; }},
    EMO_OPTIONS(EMO_OPT_ENTRY)
#undef EMO_OPT_ENTRY
};
constexpr int kOptionCount = sizeof(kOptions) / sizeof(kOptions[0]);
const OptionEntry* find_option(const char* name) {
  for (const OptionEntry& o : kOptions)
    if (strcmp(name, o.name) == 0) return &o;
  emo_set_error("unknown option '%s'", name);
  return nullptr;
}
}  // namespace

// ---- kernel timers: HIP-event pairs around selected launches, on the stream they are launched on -----------------------
// (bench.py's roofline object needs the live device time of ONE kernel that sits behind a composite entry point;
// off by default: emoasr_set_option("timers", 1))
#include <vector>
namespace {
const char* const kTimerNames[EMO_TIMER_COUNT] = {"attn_bwd_fused_kernel", "attn_bwd_dpos_kernel", "attn_fwd_kernel",
                                                  "gemm_tn_grouped_kernel", "gemm_nt_nn", "gemm_tn", "layernorm", "conv_module"};
struct TimerRec { hipEvent_t e0, e1; double flops, bytes; bool ended; };
std::vector<TimerRec> g_rec[EMO_TIMER_COUNT];
long g_timer_seen[EMO_TIMER_COUNT];  // option "timer_stride" records every n-th launch of a family only: an event pair per launch
                                     // costs ~2 % of the step for the 208-launch GEMM family; 1 in 7 is a uniform sample of its shapes
bool g_timer_open[EMO_TIMER_COUNT];
bool timer_on(int id) { return g_opt.timers == 1 || (g_opt.timers > 1 && ((g_opt.timers >> (id + 1)) & 1)); }
}  // namespace
void emo_timer_begin(int id, hipStream_t s, double flops, double bytes) {
  if (!timer_on(id)) return;
  g_timer_open[id] = (g_timer_seen[id]++ % g_opt.timer_stride) == 0;
  if (!g_timer_open[id]) return;
  TimerRec r{};
  hipEventCreate(&r.e0);
  hipEventCreate(&r.e1);
  hipEventRecord(r.e0, s);
  r.flops = flops; r.bytes = bytes; r.ended = false;
  g_rec[id].push_back(r);
}
void emo_timer_end(int id, hipStream_t s) {
  if (!timer_on(id) || !g_timer_open[id] || g_rec[id].empty() || g_rec[id].back().ended) return;
  hipEventRecord(g_rec[id].back().e1, s);
  g_rec[id].back().ended = true;
}
extern "C" int emoasr_timer_read_ex(const char* name, int* calls, double* ms, double* flops, double* bytes, int reset) {
  for (int id = 0; id < EMO_TIMER_COUNT; ++id) {
    if (strcmp(name, kTimerNames[id]) != 0) continue;
    double tot = 0.0, fl = 0.0, by = 0.0;
    int n = 0;
    for (const TimerRec& r : g_rec[id]) {
      if (!r.ended) continue;
      float t = 0.f;
      hipEventSynchronize(r.e1);
      if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) { tot += t; fl += r.flops; by += r.bytes; ++n; }
    }
    if (calls) *calls = n;
    if (ms) *ms = tot;
    if (flops) *flops = fl;
    if (bytes) *bytes = by;
    if (reset) {
      for (const TimerRec& r : g_rec[id]) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
      g_rec[id].clear();
    }
    return 0;
  }
  emo_set_error("unknown timer '%s'", name);
  return 1;
}
extern "C" int emoasr_timer_read(const char* name, int* calls, double* ms, int reset) {
  return emoasr_timer_read_ex(name, calls, ms, nullptr, nullptr, reset);
}

extern "C" const char* emoasr_last_error(void) { return g_err; }
extern "C" int emoasr_version(void) { return 1; }
extern "C" int emoasr_set_option(const char* name, int value) {
  const OptionEntry* o = find_option(name);
  if (!o) return 1;
  g_opt.*(o->field) = o->norm(value);
  return 0;
}
extern "C" int emoasr_get_option(const char* name, int* value, int* default_value) {
  const OptionEntry* o = find_option(name);
  if (!o) return 1;
  if (value) *value = g_opt.*(o->field);
  if (default_value) *default_value = o->def;
  return 0;
}
extern "C" int emoasr_option_count(void) { return kOptionCount; }
extern "C" const char* emoasr_option_name(int index) { return index >= 0 && index < kOptionCount ? kOptions[index].name : nullptr; }
