// What the host files behind the C ABI of include/misonet.h share (net.hip and the api_*.hip files, one per domain): the error
// report, per-launch profiling, the per-device lazily built table and once-latch, and the small argument checks.  Host code
// only; no kernel file includes it.
#pragma once
#include "kernels.hpp"
#include "../../include/misonet.h"

#include <atomic>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

namespace mn {

// Sets the calling thread's message (misonet_last_error) and returns `code`.  The one buffer of the library lives in net.hip.
int fail(int code, const char* fmt, ...);
#define HIPCHK(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return fail(MISONET_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

constexpr int MAX_DEV = 64;
inline int cur_dev() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MAX_DEV) d = 0;
  return d;
}

// ---- optional per-launch timing with HIP events on the caller's stream (bench.py roofline leg) ------------------
enum { PK_CONV = 0, PK_TCN, PK_MVDR, PK_OTHER, PK_N };
struct ProfRec { int kind; hipEvent_t e0, e1; };
struct Prof {
  bool on = false;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  std::vector<ProfRec> recs;
  bool overflow = false;
};
// one state per device (events belong to the device that was current when they were created); a process that drives
// several GPUs profiles each of them independently
extern Prof g_profs[MAX_DEV];
extern std::atomic<int> g_prof_any;             // fast path: no hipGetDevice per launch while nobody profiles
struct ProfScope {
  hipStream_t s; int kind; hipEvent_t e0 = nullptr, e1 = nullptr; bool active = false; Prof* pr = nullptr;
  ProfScope(hipStream_t s_, int kind_) : s(s_), kind(kind_) {
    if (!g_prof_any.load(std::memory_order_relaxed)) return;
    pr = &g_profs[cur_dev()];
    if (!pr->on) return;
    if (pr->used + 2 > pr->pool.size()) { pr->overflow = true; return; }
    e0 = pr->pool[pr->used++];
    e1 = pr->pool[pr->used++];
    active = (hipEventRecord(e0, s) == hipSuccess);
  }
  ~ProfScope() {
    if (!active) return;
    if (hipEventRecord(e1, s) == hipSuccess) pr->recs.push_back({kind, e0, e1});
  }
};

// ---- a constant table in the memory of every device that needs it -------------------------------------------------------
// get() hands out the table of the CURRENT device and builds it at the first use there: `build(&p)` runs under the lock and
// leaves the device pointer in p (dev_upload, then whatever else belongs to the first use, e.g. a kernel attribute), or
// returns an error, after which the next call tries again.  That first call allocates and copies synchronously; every later
// one is an acquire load (a reader sees the table fully built or not at all) and only queues work.
template <class T>
struct DevTable {
  std::atomic<T*> tab[MAX_DEV] = {};
  std::mutex mu;
  template <class Build>
  int get(const T** out, Build build) {
    const int d = cur_dev();
    T* p = tab[d].load(std::memory_order_acquire);
    if (!p) {
      std::lock_guard<std::mutex> lk(mu);
      p = tab[d].load(std::memory_order_acquire);
      if (!p) {
        if (const int rc = build(&p)) return rc;
        tab[d].store(p, std::memory_order_release);
      }
    }
    *out = p;
    return MISONET_OK;
  }
};
// Something that has to happen once on every device before the first asynchronous call there (a kernel attribute): once() runs
// `init` under the lock at the first use on the CURRENT device; an error is returned and the next call tries again.
struct DeviceOnce {
  std::atomic<bool> done[MAX_DEV] = {};
  std::mutex mu;
  template <class Init>
  int once(Init init) {
    const int d = cur_dev();
    if (done[d].load(std::memory_order_acquire)) return MISONET_OK;
    std::lock_guard<std::mutex> lk(mu);
    if (!done[d].load(std::memory_order_acquire)) {
      if (const int rc = init()) return rc;
      done[d].store(true, std::memory_order_release);
    }
    return MISONET_OK;
  }
};
template <class T>
int dev_upload(const std::vector<T>& host, T** out) {
  HIPCHK(hipMalloc(reinterpret_cast<void**>(out), host.size() * sizeof(T)));
  HIPCHK(hipMemcpy(*out, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  return MISONET_OK;
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------
// [a, a + na) and [b, b + nb) share a byte.  128 bits: the byte counts of a long stream do not fit 64, and an end must not wrap
inline bool ranges_overlap(const void* a, unsigned __int128 na, const void* b, unsigned __int128 nb) {
  const unsigned __int128 pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}
// false for a NaN, each of them
inline bool in_open_unit(double v) { return v > 0.0 && v < 1.0; }
inline bool pos_finite(double v) { return v > 0.0 && std::isfinite(v); }
inline bool nonneg_finite(double v) { return v >= 0.0 && std::isfinite(v); }

// ---- what one domain's file needs of another's ---------------------------------------------------------------------------
// api_frontend.hip: the STFT twiddles of the current device (builds both front-end tables at the first use there)
int get_twiddles(const float** out);
// api_array.hip: host-side check of every field (M = the number of microphones ref_ch is counted in), and the options as MvdrArgs
int bf_opts_check(const misonet_bf_opts* o, int M);
void bf_opts_apply(const misonet_bf_opts& o, MvdrArgs& a);
// api_array.hip: host-side check of every WPD field against M microphones (and against T frames when T >= 0); the options as
// WpdArgs; the kernel's attributes on the current device, set at the first call there
int wpd_opts_check(const misonet_wpd_opts* o, int M, int T);
void wpd_opts_apply(const misonet_wpd_opts& o, WpdArgs& a);
int wpd_ready();
// api_array.hip: host-side check of every cACGMM field
int cacgmm_opts_check(const misonet_cacgmm_opts* o);
// api_array.hip: host-side check of every field of the joint beamformers against M microphones and S speakers; the options as JbfArgs
int jbf_opts_check(const misonet_jbf_opts* o, int M, int S);
void jbf_opts_apply(const misonet_jbf_opts& o, JbfArgs& a);

}  // namespace mn
