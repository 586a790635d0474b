// hz_host.hpp — the host layer every .hip unit of libhz shares (csrc/units.mk
// names them): no device code.
//
//   env_int / env_pick / env_clamped / env_cuts(_n) /
//   env_p2_dcuts, Setting                                : the environment knobs
//   DevBufsT<Dev>                                        : owner of device buffers
//   streams_touched<Dev>(e)                              : voids the saved draw windows
//   launch_err(), lds_opt_in<Kernel>(bytes)              : launch helpers (HIP only)
//
// Everything above the HIP section compiles with a plain C++17 compiler
// (tests/host_driver.cpp runs it under ASan + UBSan without a GPU).
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

namespace hz_host {

// ------------------------------------------------------------------- knobs
// Every HZ_* knob of libhz goes through env_int: unset gives the default,
// anything else is what atoi makes of it ("" and garbage parse as 0).  The
// callers keep the value in a function-local static: read once per process.
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}

// `special` only if the knob parses to exactly that, `otherwise` else (unset
// included).  (name, 0, 1): on unless it parses to 0; (name, 1, 0): off
// unless it parses to 1.
inline int env_pick(const char *name, int special, int otherwise) {
  return env_int(name, otherwise) == special ? special : otherwise;
}

// the integer (or the default) clamped to [lo, hi]
inline int env_clamped(const char *name, int dflt, int lo, int hi) {
  const int v = env_int(name, dflt);
  return v < lo ? lo : v > hi ? hi : v;
}

// "a,b,c": three increasing positive multiples of 4 replace cut[]; anything
// else leaves it as it is
inline void env_cuts(const char *name, int cut[3]) {
  const char *e = getenv(name);
  int c[3];
  if (e && sscanf(e, "%d,%d,%d", &c[0], &c[1], &c[2]) == 3 && c[0] > 0 && c[1] > c[0] && c[2] > c[1] &&
      c[0] % 4 == 0 && c[1] % 4 == 0 && c[2] % 4 == 0)
    for (int k = 0; k < 3; k++) cut[k] = c[k];
}

// "a,b,...": exactly n (1..8) increasing multiples of step in [step, hi],
// comma-separated with nothing after them, replace cut[] and give true;
// anything else (unset included) leaves cut[] as it is
inline bool env_cuts_n(const char *name, int *cut, int n, int step, int hi) {
  const char *e = getenv(name);
  if (!e || n < 1 || n > 8 || step < 1) return false;
  int c[8];
  for (int k = 0; k < n; k++) {
    if (*e < '0' || *e > '9') return false;  // (no sign, no blanks)
    long v = 0;
    for (; *e >= '0' && *e <= '9'; e++)
      if ((v = v * 10 + (*e - '0')) > hi) return false;
    if (v < step || v % step || (k && v <= c[k - 1])) return false;
    c[k] = (int)v;
    if (*e++ != (k + 1 < n ? ',' : '\0')) return false;
  }
  for (int k = 0; k < n; k++) cut[k] = c[k];
  return true;
}

// whether no two neighbours of the n values are more than max_gap apart
inline bool cuts_gaps_within(const int *cut, int n, int max_gap) {
  for (int k = 0; k + 1 < n; k++)
    if (cut[k + 1] - cut[k] > max_gap) return false;
  return true;
}

// Pipeline 2's draw cuts (HZ_P2_DCUTS).  dcut[0 .. ndraw] holds the defaults
// on entry: dcut[0] = 0, the first draws of stages 2 .. ndraw, and
// dcut[ndraw] = draws, one past the last draw.  The setting lists the first
// draws of stages 2 .. ndraw (ndraw - 1 increasing values in 1 .. draws; only
// the last stage's may be `draws`, an empty stage) or, with six stages, those
// of stages 2 .. 5 alone (four values in 1 .. draws - 1): the sixth stage's
// then stays the default's, raised to the fifth's if that is later.  No stage
// may take more than max_gap draws.  True and dcut[] replaced if the setting
// is valid, else false and dcut[] as it was.
inline bool env_p2_dcuts(const char *name, int *dcut, int ndraw, int draws, int max_gap) {
  if (ndraw < 2 || ndraw > 8) return false;
  int dc[9];
  for (int k = 0; k <= ndraw; k++) dc[k] = dcut[k];
  bool got = ndraw == 6 && env_cuts_n(name, dc + 1, 5, 1, draws);
  if (!got) {
    const int n = ndraw == 6 ? 4 : ndraw - 1;
    got = env_cuts_n(name, dc + 1, n, 1, draws - 1);
    if (got && ndraw == 6 && dc[5] < dc[4]) dc[5] = dc[4];
  }
  if (!got || !cuts_gaps_within(dc, ndraw + 1, max_gap)) return false;
  for (int k = 0; k <= ndraw; k++) dcut[k] = dc[k];
  return true;
}

// A process-wide knob that a setter of the ABI can override: env_int(name,
// dflt) at the first get(), unless set() came first; set() wins from then on.
struct Setting {
  static constexpr int64_t kUnread = INT64_MIN;
  const char *name;
  int32_t dflt;
  std::atomic<int64_t> v{kUnread};
  int32_t get() {
    int64_t x = v.load(std::memory_order_relaxed);
    if (x == kUnread) {
      int64_t expect = kUnread;
      v.compare_exchange_strong(expect, (int64_t)env_int(name, dflt));
      x = v.load(std::memory_order_relaxed);
    }
    return (int32_t)x;
  }
  void set(int32_t x) { v.store(x, std::memory_order_relaxed); }
};

// ---------------------------------------------------------- device buffers
// Hands out device allocations into the caller's pointers and remembers
// them; release() frees each exactly once and nulls the caller's pointer.
// After the first request that fails, later requests do nothing and ok stays
// false until release(), so a run of get() calls needs one check at its end.
// Dev supplies the primitives: alloc(void **, bytes), fill(p, byte, bytes)
// (synchronous), fill_async(p, byte, bytes, stream) -> true on success, and
// free(p).  The owner must not move while it holds anything (it keeps the
// addresses of the caller's pointers).
template <class Dev>
struct DevBufsT {
  struct Held {
    void *p;
    void *slot;                  // the caller's pointer
    void (*clear)(void *slot);   // nulls it (as its own type)
  };
  std::vector<Held> held;
  bool ok = true;

  template <class T>
  bool get(T *&p, size_t bytes) {
    if (!ok) return false;
    void *raw = nullptr;
    if (!Dev::alloc(&raw, bytes)) return ok = false;
    p = static_cast<T *>(raw);
    held.push_back(Held{raw, &p, [](void *s) { *static_cast<T **>(s) = nullptr; }});
    return true;
  }
  template <class T>
  bool get(T *&p, size_t bytes, int byte) {  // ... filled with byte
    return get(p, bytes) && (ok = Dev::fill(p, byte, bytes));
  }
  template <class T>
  bool get(T *&p, size_t bytes, int byte, void *stream) {  // ... filled on stream
    return get(p, bytes) && (ok = Dev::fill_async(p, byte, bytes, stream));
  }
  void release() {
    for (const Held &h : held) {
      Dev::free(h.p);
      h.clear(h.slot);
    }
    held.clear();
    ok = true;
  }
};

// ----------------------------------------------------------- stream windows
// The one place an env's saved draw windows (PlyWin, hz_env.hip) are voided:
// every entry point that can move or rewrite a board's stream calls this once
// it knows e is not null, before it enqueues its own work, unless its kernel
// stores -1 to the tag of each board whose cursor it writes (hz_rollout,
// hz_play, the search's expansion: launch-bound paths).  Every board's
// window tag goes to -1 (none) by a fill in stream order, so a captured call
// voids the windows again at every replay, and a replayed per-ply launch
// reads the tags that the calls enqueued before it left: whether a window is
// trusted never depends on a value the host passed at launch.  False if the
// fill could not be enqueued.
template <class Dev, class Env>
inline bool streams_touched(Env *e) {
  return Dev::fill_async(e->pw_tag, 0xff, e->nrow * sizeof(*e->pw_tag), (void *)e->stream);
}

}  // namespace hz_host

// ---------------------------------------------------------------- HIP only
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace hz_host {

struct HipDev {
  static bool alloc(void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess; }
  static bool fill(void *p, int byte, size_t bytes) { return hipMemset(p, byte, bytes) == hipSuccess; }
  static bool fill_async(void *p, int byte, size_t bytes, void *stream) {
    return hipMemsetAsync(p, byte, bytes, (hipStream_t)stream) == hipSuccess;
  }
  static void free(void *p) { (void)hipFree(p); }
};
using DevBufs = DevBufsT<HipDev>;

inline int launch_err() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// The opt-in to more than 64 KB of dynamic LDS, once per (kernel
// instantiation, device): 0, or 1 if the device cannot be told (devices 0-63).
template <auto Kernel>
inline int lds_opt_in(size_t bytes) {
  static std::atomic<uint64_t> init_mask{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1;
  if (!(init_mask.load(std::memory_order_acquire) >> dev & 1)) {
    if (hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
        hipSuccess)
      return 1;
    init_mask.fetch_or(1ull << dev, std::memory_order_release);
  }
  return 0;
}

}  // namespace hz_host
#endif  // __HIPCC__
