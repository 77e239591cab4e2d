// hermite_block_stub.cpp — TEST INFRASTRUCTURE (tests/test_hermite_block_host_sanitizers.py): a host-only stand-in for the launch
// functions of hermite_block.hip, linked beside hip_stub.cpp, jerk_stub.cpp (the jerk pass the block step evaluates with, rows and
// points) and hermite_stub.cpp so that hermite_block.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.
// hip_stub.cpp's streams are synchronous, so every function executes at launch.
// The stand-in pushes the scheme's own arithmetic and level rules (hermite_block_args.hpp, hermite_args.hpp) through the REAL BlockArgs —
// the own slice's offset into pos[cur], the base, the ticks and levels, the tiles' counts, the active list, the three query buffers and
// the evaluations indexed by the list — so ASan sees every pointer the host computed and every index a list carries, and refuses
// what the real launch functions refuse, by the same predicates.  The compaction is the plain ascending scan, which is what the
// ballots on the device amount to; it stores through the tiles' counts all the same, so a wrong count is found out.  It says nothing
// about the kernels themselves (the GPU tests do).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../mini_nbody_amd/csrc/hermite_block_args.hpp"
#include "stub_common.hpp"

namespace {

using nbh::Coefficients;
using nbhb::BlockArgs;
using nbhb::NextTime;
using stub::W4;

template <typename T> T unit_of(const BlockArgs& a) { return sizeof(T) == 8 ? (T)a.unit_d : (T)a.unit; }
template <typename T> T step_of(const BlockArgs& a, int p) { return (T)(a.tau - a.t0[p]) * unit_of<T>(a); }
bool reaches(const BlockArgs& a, int p) { return a.t0[p] + nbhb::ticks_of(a.level[p], a.levels) == a.tau; }

template <typename T>
void init(const BlockArgs& a) {
  typedef W4<T> V;
  for (int p = 0; p < a.rows; ++p) {
    ((V*)a.x0)[p] = ((const V*)a.pos)[p];
    ((V*)a.v0)[p] = ((const V*)a.vel)[p];
    a.t0[p] = 0;
    a.level[p] = nbhb::wanted_level(((const V*)a.a0)[p], ((const V*)a.j0)[p], a.eta2, a.lim, a.levels);
  }
}

template <typename T>
void predict(const BlockArgs& a) {
  typedef W4<T> V;
  const int tiles = (a.rows + nbd::kLanes - 1) / nbd::kLanes;
  for (int b = 0; b < tiles; ++b) a.counts[b] = 0;
  for (int p = 0; p < a.rows; ++p) {
    const Coefficients<T> c = nbh::coefficients_of(step_of<T>(a, p));
    const V x0 = ((const V*)a.x0)[p], v0 = ((const V*)a.v0)[p], a0 = ((const V*)a.a0)[p], j0 = ((const V*)a.j0)[p];
    V xp = x0, vp = v0;
    xp.x = std::fma(c.c3, j0.x, std::fma(c.c2, a0.x, std::fma(c.h, v0.x, x0.x)));
    xp.y = std::fma(c.c3, j0.y, std::fma(c.c2, a0.y, std::fma(c.h, v0.y, x0.y)));
    xp.z = std::fma(c.c3, j0.z, std::fma(c.c2, a0.z, std::fma(c.h, v0.z, x0.z)));
    vp.x = std::fma(c.c2, j0.x, std::fma(c.h, a0.x, v0.x));
    vp.y = std::fma(c.c2, j0.y, std::fma(c.h, a0.y, v0.y));
    vp.z = std::fma(c.c2, j0.z, std::fma(c.h, a0.z, v0.z));
    ((V*)a.pos)[p] = xp;
    ((V*)a.vel)[p] = vp;
    if (reaches(a, p)) a.counts[p / nbd::kLanes] += 1;
  }
}

template <typename T>
void compact(const BlockArgs& a) {
  typedef W4<T> V;
  const int tiles = (a.rows + nbd::kLanes - 1) / nbd::kLanes;
  int before = 0;
  for (int b = 0; b < tiles; ++b) {
    int at = before;
    for (int p = b * nbd::kLanes; p < std::min((b + 1) * nbd::kLanes, a.rows); ++p) {
      if (!reaches(a, p)) continue;
      a.active[at] = p;   // (unchecked against m on purpose: the host sized the buffers for what it read from the next-time word)
      ((V*)a.q_points)[at] = ((const V*)a.pos)[p];
      ((V*)a.q_vel)[at] = ((const V*)a.vel)[p];
      a.q_skip[at] = a.first + p;
      ++at;
    }
    before += a.counts[b];
  }
}

template <typename T>
void correct(const BlockArgs& a) {
  typedef W4<T> V;
  for (int q = 0; q < a.m; ++q) {
    const int p = a.active[q];
    const Coefficients<T> c = nbh::coefficients_of(step_of<T>(a, p));
    const V x0 = ((const V*)a.x0)[p], v0 = ((const V*)a.v0)[p];
    const V a0 = ((const V*)a.a0)[p], j0 = ((const V*)a.j0)[p], a1 = ((const V*)a.a1)[q], j1 = ((const V*)a.j1)[q];
    V x1 = x0, v1 = v0;
    auto cv = [&](T v, T a0k, T a1k, T j0k, T j1k) { const T dj = j0k - j1k, sa = a0k + a1k; return std::fma(c.c12, dj, std::fma(c.hh, sa, v)); };
    auto cx = [&](T x, T v, T w, T a0k, T a1k) { const T da = a0k - a1k, sv = v + w; return std::fma(c.c12, da, std::fma(c.hh, sv, x)); };
    v1.x = cv(v0.x, a0.x, a1.x, j0.x, j1.x);
    v1.y = cv(v0.y, a0.y, a1.y, j0.y, j1.y);
    v1.z = cv(v0.z, a0.z, a1.z, j0.z, j1.z);
    x1.x = cx(x0.x, v0.x, v1.x, a0.x, a1.x);
    x1.y = cx(x0.y, v0.y, v1.y, a0.y, a1.y);
    x1.z = cx(x0.z, v0.z, v1.z, a0.z, a1.z);
    ((V*)a.x0)[p] = x1;
    ((V*)a.v0)[p] = v1;
    ((V*)a.a0)[p] = a1;
    ((V*)a.j0)[p] = j1;
    ((V*)a.pos)[p] = x1;
    ((V*)a.vel)[p] = v1;
    a.t0[p] = a.tau;
    a.level[p] = nbhb::next_level(a.level[p], nbhb::wanted_level(a1, j1, a.eta2, a.lim, a.levels), a.tau, a.levels);
  }
}

}  // namespace

namespace nbl {
int launch_hermite_block_init_kernel(int fp64, hipStream_t, const BlockArgs& a) {
  if (nbhb::bad_block_rows(a)) return (int)hipErrorInvalidValue;
  if (fp64) init<double>(a); else init<float>(a);
  return 0;
}
int launch_hermite_block_predict_kernel(int fp64, hipStream_t, const BlockArgs& a) {
  if (nbhb::bad_block_predict(a)) return (int)hipErrorInvalidValue;
  if (fp64) predict<double>(a); else predict<float>(a);
  return 0;
}
int launch_hermite_block_next_kernel(hipStream_t, const long long* t0, const int* level, int rows, int levels, NextTime* out) {
  if (nbd::bad_row_reduce(rows, out, t0 && level) || levels < 1 || levels > nbhb::kMaxLevels) return (int)hipErrorInvalidValue;
  NextTime w = {nbhb::kNoTick, 0, 0};
  for (int r = 0; r < rows; ++r) {
    const long long next = t0[r] + nbhb::ticks_of(level[r], levels);
    if (next < w.tick) { w.tick = next; w.count = 1; }
    else if (next == w.tick) ++w.count;
  }
  *out = w;
  return 0;
}
int launch_hermite_block_compact_kernel(int fp64, hipStream_t, const BlockArgs& a) {
  if (nbhb::bad_block_compact(a)) return (int)hipErrorInvalidValue;
  if (fp64) compact<double>(a); else compact<float>(a);
  return 0;
}
int launch_hermite_block_correct_kernel(int fp64, hipStream_t, const BlockArgs& a) {
  if (nbhb::bad_block_correct(a)) return (int)hipErrorInvalidValue;
  if (fp64) correct<double>(a); else correct<float>(a);
  return 0;
}
}  // namespace nbl
