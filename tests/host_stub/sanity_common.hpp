// sanity_common.hpp — TEST INFRASTRUCTURE: what the sanitizer drivers (host_sanity.cpp, point_sums_sanity.cpp, neighbors_sanity.cpp and their siblings) share.
// A driver defines SANITY_NAME, the name its messages carry, before it includes this.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <vector>

#include "../../include/nbody.h"

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
