// sanity_common.hpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): what the sanitizer drivers (host_sanity.cpp and the passes' *_sanity.cpp) share:
// CHECK / OK / SHUTDOWN, the failure sweep, and the kit of the pass drivers — a pass's two environment variables, the device counts
// and sizes every driver walks, the fixture of bodies, points and skip indices with the queries the stub rule sees of them, the mark
// of an untouched output, and the refused row windows and skip indices.
// A driver defines SANITY_NAME, the name its messages carry, before it includes this.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/nbody.h"
#include "stub_rule.hpp"

extern "C" long hip_stub_live(int kind);               // hip_stub.cpp: outstanding 0 device allocations, 1 pinned, 2 events, 3 streams, 4 graphs, 5 graph execs
extern "C" void hip_stub_fail_nth(int k);              // the k-th creating call from now fails once (0: disarm)
extern "C" int hip_stub_fail_pending(void);            // > 0: the armed failure has not been reached

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, SANITY_NAME ": line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)
#define OK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, SANITY_NAME ": line %d: %s = %d (%s)\n", __LINE__, #call, rc_, nbody_error_string(rc_)); exit(1); } } while (0)

// nbody_shutdown() leaves nothing of any kind behind
static void shutdown_at(int line) {
  nbody_shutdown();
  for (int kind = 0; kind < 6; ++kind)
    if (hip_stub_live(kind)) { fprintf(stderr, SANITY_NAME ": line %d: %ld of kind %d live after nbody_shutdown\n", line, hip_stub_live(kind), kind); exit(1); }
}
#define SHUTDOWN() shutdown_at(__LINE__)

template <typename T> int upload(std::vector<T>& pos, std::vector<T>& vel);
template <> inline int upload<float>(std::vector<float>& pos, std::vector<float>& vel) { BodySystem b = {pos.data(), vel.data()}; return nbody_upload(&b); }
template <> inline int upload<double>(std::vector<double>& pos, std::vector<double>& vel) { BodySystemD b = {pos.data(), vel.data()}; return nbody_upload_d(&b); }

// One entry point under creation-failure injection.  `setup` brings a fresh context to the point before the call (no injection), `call`
// is the call, `verify` checks its results.  k = 1, 2, 3, ...: the k-th creating call (hipMalloc, hipHostMalloc, hipEventCreate*,
// hipStreamCreate*, hipGraphInstantiate) inside `call` fails, until the call no longer reaches the armed failure.  Every k is walked (no
// stride).  A failed call must say so, nbody_shutdown() must then leave nothing, and the same call without injection must then work.
// Returns the number of creating calls the call makes.
static int sweep(const char* name, const std::function<void()>& setup, const std::function<int()>& call, const std::function<void()>& verify) {
  for (int k = 1;; ++k) {
    setup();
    hip_stub_fail_nth(k);
    const int rc = call();
    const bool reached = hip_stub_fail_pending() == 0;
    hip_stub_fail_nth(0);
    if (reached && rc == 0) { fprintf(stderr, SANITY_NAME ": %s: creating call %d failed and the call returned 0\n", name, k); exit(1); }
    if (!reached) {
      if (rc) { fprintf(stderr, SANITY_NAME ": %s: %d (%s) without an injected failure\n", name, rc, nbody_error_string(rc)); exit(1); }
      verify();
      SHUTDOWN();
      return k - 1;
    }
    SHUTDOWN();
    setup();
    const int rc2 = call();
    if (rc2) { fprintf(stderr, SANITY_NAME ": %s: %d (%s) after a failed attempt at creating call %d\n", name, rc2, nbody_error_string(rc2), k); exit(1); }
    verify();
    SHUTDOWN();
  }
}

// ---- the pass drivers' kit ----

static void set_env(const char* name, const char* value) { if (value) setenv(name, value, 1); else unsetenv(name); }
// the two variables that steer a pass's source split; a null value unsets the variable (the automatic split, the default bound)
struct SplitEnv {
  std::string split, scratch_mb;
  void set(const char* split_value, const char* mb_value) const { set_env(split.c_str(), split_value); set_env(scratch_mb.c_str(), mb_value); }
};
// fn under every split value in turn, the scratch bound unset; both unset afterwards
static void for_splits(const SplitEnv& env, std::initializer_list<const char*> splits, const std::function<void()>& fn) {
  for (const char* split : splits) { env.set(split, nullptr); fn(); }
  env.set(nullptr, nullptr);
}

// the stub offers three devices (tests/test_host_sanitizers.py sets STUB_DEVICES=3)
static bool three_devices() { const char* e = getenv("STUB_DEVICES"); return e && atoi(e) >= 3; }
static void for_device_counts(const std::function<void(int)>& fn) {
  fn(1);
  if (three_devices()) fn(3);
}
// The sizes of a driver's shapes section: fp32 at every n on one device and, from three bodies on, on three with ragged slices; fp64 at
// the last (largest) n on one device and at 1000 = 333 + 333 + 334 on three.
static void for_sizes(std::initializer_list<int> ns, void (*fp32)(int n, int ngpus), void (*fp64)(int n, int ngpus)) {
  for (int n : ns) {
    fp32(n, 1);
    if (three_devices() && n >= 3) fp32(n, 3);
  }
  fp64(*(ns.end() - 1), 1);
  if (three_devices()) fp64(1000, 3);
}
static const int kShapeM[] = {1, 255, 256, 257, 5000};   // the query counts of a shapes section: around one workgroup's 256, and many

// outputs are filled with kMark before a call; what the call must not write still holds it afterwards
constexpr int kMark = -77;
template <class V> void mark(V& v) { std::fill(v.begin(), v.end(), (typename V::value_type)kMark); }
template <class V> bool nothing_beyond(const V& v, size_t k) {
  for (; k < v.size(); ++k) if (v[k] != (typename V::value_type)kMark) return false;
  return true;
}

// what every rows form refuses of a window (first, count) of n rows, c being a legal count; what every points form refuses in skip
struct Window { int first, count; };
static std::vector<Window> refused_windows(int n, int c) { return {{-1, c}, {0, 0}, {0, -4}, {n, 1}, {n - 200, 201}, {1 << 30, 1 << 30}}; }
static std::vector<int> refused_skips(int n) { return {n, -2, 1 << 30}; }

// n bodies {x, y, z, w}, zero velocities, and the context that holds them; a driver fills pos
template <typename T>
struct System {
  int n;
  std::vector<T> pos, vel;
  explicit System(int n_) : n(n_), pos((size_t)n_ * 4), vel((size_t)n_ * 4, (T)0) {}
  void set(std::vector<T>& words, int at, T x, T y, T z, T w) { T* p = &words[4 * (size_t)at]; p[0] = x; p[1] = y; p[2] = z; p[3] = w; }
  void open(int ngpus) { OK(nbody_init(n, ngpus, sizeof(T) == 8, 0)); OK(upload<T>(pos, vel)); }
};
// The fixture of the point passes: bodies, m points and their skip indices, small integers everywhere so that every value of a stub
// is exact in either precision.  w steers the stub rule: j % 977 for a body as a row, p, its index in the caller's array, for a point.
template <typename T>
struct Fixture : System<T> {
  int m;
  std::vector<T> pts;
  std::vector<int> skip;
  Fixture(int n_, int m_) : System<T>(n_), m(m_), pts((size_t)m_ * 4), skip((size_t)m_) {
    for (int j = 0; j < n_; ++j) this->set(this->pos, j, (T)((j * 37) % 101), (T)(j % 7), (T)1, (T)(j % 977));
    for (int p = 0; p < m; ++p) {
      this->set(pts, p, (T)(p % 17), (T)(p % 5), (T)3, (T)p);
      skip[(size_t)p] = p % 3 == 0 ? -1 : (int)(((long long)p * 7919) % n_);
    }
  }
  // what the stub rule sees of a query: x, the steering w, the excluded body
  struct Q { T x, w; int sk; };
  Q row(int i) const { return {this->pos[4 * (size_t)i], this->pos[4 * (size_t)i + 3], i}; }
  Q point(int p, bool with_skip) const { return {pts[4 * (size_t)p], pts[4 * (size_t)p + 3], with_skip ? skip[(size_t)p] : -1}; }
  std::vector<int> skip_with(int at, int value) const { std::vector<int> sk = skip; sk[(size_t)at] = value; return sk; }
};
