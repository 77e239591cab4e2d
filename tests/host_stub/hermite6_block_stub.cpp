// hermite6_block_stub.cpp — TEST INFRASTRUCTURE (tests/test_hermite6_block_host_sanitizers.py): a host-only stand-in for the launch
// functions of hermite6_block.hip, linked beside hip_stub.cpp, snap_stub.cpp (the snap pass the block step evaluates with, rows and
// points), hermite_stub.cpp, hermite_block_stub.cpp (the next-time reduction, which the sixth-order scheduler reuses) and
// hermite6_stub.cpp so that hermite6_block.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.  hip_stub.cpp's streams
// are synchronous, so every function executes at launch.
// The stand-in pushes the scheme's own arithmetic and level rules (hermite6_args.hpp, hermite_block_args.hpp) through the REAL
// Block6Args — the own slice's offset into pos[cur], the base with its snap and crackle words, the predicted accelerations, the ticks and
// levels, the tiles' counts, the active list, the four query buffers and the three evaluations indexed by the list — so ASan sees every
// pointer the host computed and every index a list carries, and refuses what the real launch functions refuse, by the same
// predicates.  The compaction is the plain ascending scan, which is what the ballots on the device amount to; it stores through the
// tiles' counts all the same, so a wrong count is found out.  It says nothing about the kernels themselves (the GPU tests do).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../mini_nbody_amd/csrc/hermite6_block_args.hpp"
#include "stub_common.hpp"

namespace {

using nbh6::Coefficients6;
using nbh6b::Block6Args;
using nbhb::BlockArgs;
using stub::W4;

template <typename T> T unit_of(const BlockArgs& a) { return sizeof(T) == 8 ? (T)a.unit_d : (T)a.unit; }
template <typename T> T step_of(const BlockArgs& a, int p) { return (T)(a.tau - a.t0[p]) * unit_of<T>(a); }
bool reaches(const BlockArgs& a, int p) { return a.t0[p] + nbhb::ticks_of(a.level[p], a.levels) == a.tau; }
template <typename T> T* at(W4<T>& w, int c) { return c == 0 ? &w.x : c == 1 ? &w.y : &w.z; }
template <typename T> T of(const W4<T>& w, int c) { return c == 0 ? w.x : c == 1 ? w.y : w.z; }

template <typename T>
void init(const Block6Args& a) {
  typedef W4<T> V;
  for (int p = 0; p < a.b.rows; ++p) {
    ((V*)a.b.x0)[p] = ((const V*)a.b.pos)[p];
    ((V*)a.b.v0)[p] = ((const V*)a.b.vel)[p];
    a.b.t0[p] = 0;
    a.b.level[p] = nbhb::wanted_level(((const V*)a.b.a0)[p], ((const V*)a.b.j0)[p], a.b.eta2, a.b.lim, a.b.levels);
  }
}

template <typename T>
void predict(const Block6Args& a) {
  typedef W4<T> V;
  const int tiles = (a.b.rows + nbd::kLanes - 1) / nbd::kLanes;
  for (int b = 0; b < tiles; ++b) a.b.counts[b] = 0;
  for (int p = 0; p < a.b.rows; ++p) {
    const Coefficients6<T> c = nbh6::coefficients6_of(step_of<T>(a.b, p));
    const V x0 = ((const V*)a.b.x0)[p], v0 = ((const V*)a.b.v0)[p], a0 = ((const V*)a.b.a0)[p], j0 = ((const V*)a.b.j0)[p];
    const V s0 = ((const V*)a.s0)[p], c0 = ((const V*)a.c0)[p];
    V xp = x0, vp = v0, ap = a0;
    for (int k = 0; k < 3; ++k) {
      const T x = of(x0, k), v = of(v0, k), g = of(a0, k), j = of(j0, k), s = of(s0, k), q = of(c0, k);
      *at(xp, k) = std::fma(c.c5, q, std::fma(c.c4, s, std::fma(c.c3, j, std::fma(c.c2, g, std::fma(c.h, v, x)))));
      *at(vp, k) = std::fma(c.c4, q, std::fma(c.c3, s, std::fma(c.c2, j, std::fma(c.h, g, v))));
      *at(ap, k) = std::fma(c.c3, q, std::fma(c.c2, s, std::fma(c.h, j, g)));
    }
    ((V*)a.b.pos)[p] = xp;
    ((V*)a.b.vel)[p] = vp;
    ((V*)a.ap)[p] = ap;
    if (reaches(a.b, p)) a.b.counts[p / nbd::kLanes] += 1;
  }
}

template <typename T>
void compact(const Block6Args& a) {
  typedef W4<T> V;
  const int tiles = (a.b.rows + nbd::kLanes - 1) / nbd::kLanes;
  int before = 0;
  for (int b = 0; b < tiles; ++b) {
    int at = before;
    for (int p = b * nbd::kLanes; p < std::min((b + 1) * nbd::kLanes, a.b.rows); ++p) {
      if (!reaches(a.b, p)) continue;
      a.b.active[at] = p;   // (unchecked against m on purpose: the host sized the buffers for what it read from the next-time word)
      ((V*)a.b.q_points)[at] = ((const V*)a.b.pos)[p];
      ((V*)a.b.q_vel)[at] = ((const V*)a.b.vel)[p];
      ((V*)a.q_acc)[at] = ((const V*)a.ap)[p];
      a.b.q_skip[at] = a.b.first + p;
      ++at;
    }
    before += a.b.counts[b];
  }
}

template <typename T>
void correct(const Block6Args& a) {
  typedef W4<T> V;
  for (int q = 0; q < a.b.m; ++q) {
    const int p = a.b.active[q];
    const Coefficients6<T> c = nbh6::coefficients6_of(step_of<T>(a.b, p));
    const V x0 = ((const V*)a.b.x0)[p], v0 = ((const V*)a.b.v0)[p];
    const V a0 = ((const V*)a.b.a0)[p], j0 = ((const V*)a.b.j0)[p], s0 = ((const V*)a.s0)[p];
    const V a1 = ((const V*)a.b.a1)[q], j1 = ((const V*)a.b.j1)[q], s1 = ((const V*)a.s1)[q];
    V x1 = x0, v1 = v0, c1 = a1;
    for (int k = 0; k < 3; ++k) {
      const T ss = of(s0, k) + of(s1, k), dj = of(j0, k) - of(j1, k), sa = of(a0, k) + of(a1, k);
      const T sj = of(j0, k) + of(j1, k), da = of(a0, k) - of(a1, k);
      const T v = std::fma(c.c120, ss, std::fma(c.c10, dj, std::fma(c.hh, sa, of(v0, k))));
      const T sv = of(v0, k) + v;
      *at(v1, k) = v;
      *at(x1, k) = std::fma(c.c120, sj, std::fma(c.c10, da, std::fma(c.hh, sv, of(x0, k))));
      const T d1 = of(a1, k) - of(a0, k);
      const T e1 = (T)60 * d1, p24 = (T)24 * of(j0, k), m3 = (T)-3 * of(s0, k);
      const T e2 = std::fma((T)36, of(j1, k), p24), e3 = std::fma((T)9, of(s1, k), m3);
      *at(c1, k) = c.r * std::fma(c.r, std::fma(c.r, e1, -e2), e3);
    }
    ((V*)a.b.x0)[p] = x1;
    ((V*)a.b.v0)[p] = v1;
    ((V*)a.b.a0)[p] = a1;
    ((V*)a.b.j0)[p] = j1;
    ((V*)a.s0)[p] = s1;
    ((V*)a.c0)[p] = c1;
    ((V*)a.b.pos)[p] = x1;
    ((V*)a.b.vel)[p] = v1;
    a.b.t0[p] = a.b.tau;
    a.b.level[p] = nbhb::next_level(a.b.level[p], nbhb::wanted_level(a1, j1, a.b.eta2, a.b.lim, a.b.levels), a.b.tau, a.b.levels);
  }
}

}  // namespace

namespace nbl {
int launch_hermite6_block_init_kernel(int fp64, hipStream_t, const Block6Args& a) {
  if (nbh6b::bad_block6_rows(a)) return (int)hipErrorInvalidValue;
  if (fp64) init<double>(a); else init<float>(a);
  return 0;
}
int launch_hermite6_block_predict_kernel(int fp64, hipStream_t, const Block6Args& a) {
  if (nbh6b::bad_block6_predict(a)) return (int)hipErrorInvalidValue;
  if (fp64) predict<double>(a); else predict<float>(a);
  return 0;
}
int launch_hermite6_block_compact_kernel(int fp64, hipStream_t, const Block6Args& a) {
  if (nbh6b::bad_block6_compact(a)) return (int)hipErrorInvalidValue;
  if (fp64) compact<double>(a); else compact<float>(a);
  return 0;
}
int launch_hermite6_block_correct_kernel(int fp64, hipStream_t, const Block6Args& a) {
  if (nbh6b::bad_block6_correct(a)) return (int)hipErrorInvalidValue;
  if (fp64) correct<double>(a); else correct<float>(a);
  return 0;
}
}  // namespace nbl
