// stub_common.hpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): the skeleton the passes' stubs share.  A stub includes its
// pass's real *_args.hpp (its scratch layout functions and launch guards are the point of the exercise), then this.
#pragma once
#include <atomic>

#include "../../mini_nbody_amd/csrc/diag_pass.hpp"
#include "stub_rule.hpp"

static_assert(stub::kBlock == nbd::kSrcBlock, "stub_rule.hpp's block is the library's");

namespace stub {

// the preamble of a distance query, for any argument block with src, points, skip and first (nbd::query_of on the device): the query
// word — points[p], or in the rows form (a.points == null) source first + p — and the body it leaves out: skip[p], -1 without a skip
// array, in the rows form itself
template <typename T>
struct Query { W4<T> q; int sk; };
template <typename T, class A>
inline Query<T> query_of(const A& a, int p) {
  const W4<T>* src = (const W4<T>*)a.src;
  if (!a.points) return {src[a.first + p], a.first + p};
  return {((const W4<T>*)a.points)[p], a.skip ? a.skip[p] : -1};
}

// the walk of a launch: fn(p, y, b0, b1) for every query p and every chunk y, whose blocks are [b0, b1)
template <class A, class F>
inline void for_each_chunk(const A& a, F fn) {
  for (int p = 0; p < a.m; ++p)
    for (int y = 0; y < a.chunks; ++y) fn(p, y, y * a.chunk_blocks, std::min((y + 1) * a.chunk_blocks, a.n_blocks));
}

}  // namespace stub

// a launch counter g_<name> and the accessor `long <name>(void)` a driver declares extern "C"
#define STUB_COUNTER(name)                 \
  static std::atomic<long> g_##name{0};    \
  extern "C" long name(void) { return g_##name.load(); }
