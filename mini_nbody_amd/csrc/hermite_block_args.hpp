// hermite_block_args.hpp — what hermite_block.cpp (host) and hermite_block.hip (device) agree on: the argument block of the block-step
// scheduler's kernels, the word of the next-time reduction, the wanted level of a row and the launch functions of hermite_block.hip.
// Like hermite_args.hpp, whose predictor, corrector, coefficients_of and ratio_of it uses unchanged, it stays apart from nbody_args.hpp,
// the force path's hashed kernel source.
//
// The scheme (include/nbody.h, "individual block time steps") in short: time is integer ticks of unit = dt_max * 2^-(levels - 1); row i
// carries a tick t0_i, a level k_i and its base (x0, v0, a0, j0) at t0_i; its step is s_i = 2^(levels - 1 - k_i) ticks.  A sub-step
// predicts EVERY own row from its base to tau, the smallest next time of the system, evaluates the rows that reach tau (the jerk points
// pass of point_sums.hip over queries gathered here) and corrects those rows alone.
#pragma once
#include <hip/hip_runtime.h>

#include "hermite_args.hpp"

namespace nbhb {

constexpr int kMaxLevels = 24;   // (tau - t0_i) stays below 2^23 + 1: exact in binary32

// what the next-time kernel leaves per device or rank: the smallest t0_i + s_i of its rows and how many rows reach it; no row:
// tick = kNoTick, count = 0.  Exact integers: the host folds the ranks' words in any order
struct NextTime { long long tick; int count, pad; };
constexpr long long kNoTick = 0x7fffffffffffffffLL;

struct BlockArgs {
  void* pos;          // [rows] position words of the local's own slice of the live buffer: the predicted words, then the corrected ones
  void* vel;          // [rows] velocity words of the own slice likewise
  void* x0;           // [rows] the base: position and ...
  void* v0;           // ... velocity words at t0_i, ...
  void* a0;           // ... and the {ax, ay, az, 0}, ...
  void* j0;           // ... {jx, jy, jz, 0} words there
  const void* a1;     // [m] the active rows' evaluation at tau, in the order of `active` (correct only)
  const void* j1;
  long long* t0;      // [rows] ticks
  int* level;         // [rows] levels
  int* counts;        // [ceil(rows / kLanes)] active rows per workgroup tile of a sub-step: predict writes them, compact reads them
  int* active;        // [m] the own rows that reach tau, ascending: compact writes them, correct reads them
  void* q_points;     // [m] the queries of the jerk points pass, compact writes them: the active rows' predicted position words, ...
  void* q_vel;        // ... velocity words ...
  int* q_skip;        // ... and global indices
  int rows, first;    // own rows, global index of row 0
  int m;              // active rows of this sub-step on this local (correct; compact's stores stay below it)
  int levels;
  long long tau;      // the tick of the sub-step
  float unit;         // the tick in an fp32 context ...
  double unit_d;      // ... and in an fp64 one
  double eta2;        // eta * eta, binary64, formed on the host from the T value of eta
  double lim[kMaxLevels];   // lim[k] = (dt_max * 2^-k)^2 in binary64
};

// The wanted level of a row from its (a, j), binary64, no sqrt: q = ratio_of(a, j); q not < +inf (NaN or +inf: a lone body, zero jerk):
// level 0; else the smallest k with lim[k] <= eta2 * q, levels - 1 where there is none.
template <typename V4>
__host__ __device__ inline int wanted_level(const V4 a, const V4 j, double eta2, const double* lim, int levels) {
  const double q = nbh::ratio_of(a, j);
  if (!(q < (double)__builtin_huge_valf())) return 0;
  const double e = eta2 * q;
  for (int k = 0; k < levels; ++k)
    if (lim[k] <= e) return k;
  return levels - 1;
}
// ... and the level a corrected row goes on with: finer at once (always aligned), coarser by one doubling and only onto an aligned time
__host__ __device__ inline int next_level(int k, int want, long long tau, int levels) {
  if (want > k) return want;
  if (want < k && (tau & ((1LL << (levels - k)) - 1)) == 0) return k - 1;
  return k;
}
// the ticks of a step on level k
__host__ __device__ inline long long ticks_of(int k, int levels) { return 1LL << (levels - 1 - k); }

// what the launches refuse
inline bool bad_block_rows(const BlockArgs& a) {
  return a.rows <= 0 || a.levels < 1 || a.levels > kMaxLevels || !a.pos || !a.vel || !a.x0 || !a.v0 || !a.a0 || !a.j0 || !a.t0 || !a.level;
}
inline bool bad_block_predict(const BlockArgs& a) { return bad_block_rows(a) || !a.counts || a.tau < 1; }
inline bool bad_block_compact(const BlockArgs& a) {
  return bad_block_predict(a) || a.m < 1 || a.m > a.rows || a.first < 0 || !a.active || !a.q_points || !a.q_vel || !a.q_skip;
}
inline bool bad_block_correct(const BlockArgs& a) { return bad_block_rows(a) || a.m < 1 || a.m > a.rows || a.tau < 1 || !a.active || !a.a1 || !a.j1; }

}  // namespace nbhb

namespace nbl {
// all return a hipError_t as int (0 = launched)
// init: base := the own rows' state, t0 := 0, level := wanted_level(a0, j0); one row per lane
int launch_hermite_block_init_kernel(int fp64, hipStream_t stream, const nbhb::BlockArgs& a);
// every own row predicted from its base to a.tau into pos / vel (h_i = (T)(tau - t0_i) * unit, coefficients_of(h_i) per row), and the
// number of rows that reach tau per tile of kLanes rows into counts
int launch_hermite_block_predict_kernel(int fp64, hipStream_t stream, const nbhb::BlockArgs& a);
// {min over the rows of t0 + s, rows that reach it} into *out; one workgroup, rows == 0 allowed (kNoTick, 0)
int launch_hermite_block_next_kernel(hipStream_t stream, const long long* t0, const int* level, int rows, int levels, nbhb::NextTime* out);
// the rows that reach a.tau, ascending, into active, and their predicted words and global indices into the query buffers (after predict)
int launch_hermite_block_compact_kernel(int fp64, hipStream_t stream, const nbhb::BlockArgs& a);
// the active rows corrected with their own h_i: base := (x1, v1, a1, j1), t0 := tau, pos / vel := (x1, v1), level := next_level
int launch_hermite_block_correct_kernel(int fp64, hipStream_t stream, const nbhb::BlockArgs& a);
}  // namespace nbl
