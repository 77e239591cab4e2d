// hermite6_block_args.hpp — what hermite6_block.cpp (host) and hermite6_block.hip (device) agree on: the argument block of the
// sixth-order block-step scheduler's kernels and their launch functions.  The level rules, the tick arithmetic, the next-time word and
// its kernel are hermite_block_args.hpp's, used unchanged (wanted_level on |a|^2 / |j|^2, next_level, ticks_of, NextTime, kNoTick); the
// coefficients of a step are hermite6_args.hpp's coefficients6_of, evaluated per row on the device.  Like both it stays apart from
// nbody_args.hpp, the force path's hashed kernel source.
//
// The scheme (include/nbody.h, "sixth-order individual block time steps") in short: time is integer ticks of unit = dt_max *
// 2^-(levels - 1); row i carries a tick t0_i, a level k_i and its base (x0, v0, a0, j0, s0, c0) at t0_i, c the crackle.  A sub-step
// predicts EVERY own row from its base to tau, the smallest next time of the system — (xp, vp, ap), hermite6_args.hpp's three fma
// chains with h_i = (T)(tau - t0_i) * unit —, evaluates the rows that reach tau (the snap points pass of point_sums.hip over queries
// gathered here) and corrects those rows alone with their own h_i: hermite6_args.hpp's v1, x1 and crackle c1 with r = 1 / h_i.
#pragma once
#include <hip/hip_runtime.h>

#include "hermite6_args.hpp"
#include "hermite_block_args.hpp"

namespace nbh6b {

struct Block6Args {
  nbhb::BlockArgs b;   // the fourth-order scheduler's block, every member with its meaning there: pos, vel, the base (x0, v0, a0, j0), the
                       // evaluations (a1, j1), t0, level, counts, active, q_points, q_vel, q_skip, rows, first, m, levels, tau, unit, eta2, lim
  void* s0;            // [rows] the base's {sx, sy, sz, 0} words ...
  void* c0;            // ... and crackle words {cx, cy, cz, 0} (zeros at the start of a call)
  void* ap;            // [rows] predicted acceleration words: predict writes them (the snap pass's third source stream once gathered)
  const void* s1;      // [m] the active rows' snap at tau, in the order of `active` (correct only)
  void* q_acc;         // [m] the queries' predicted acceleration words: compact writes them
};

// what the launches refuse
inline bool bad_block6_rows(const Block6Args& a) { return nbhb::bad_block_rows(a.b) || !a.s0 || !a.c0; }
inline bool bad_block6_predict(const Block6Args& a) { return nbhb::bad_block_predict(a.b) || !a.s0 || !a.c0 || !a.ap; }
inline bool bad_block6_compact(const Block6Args& a) { return nbhb::bad_block_compact(a.b) || !a.ap || !a.q_acc; }
inline bool bad_block6_correct(const Block6Args& a) { return nbhb::bad_block_correct(a.b) || !a.s0 || !a.c0 || !a.s1; }

}  // namespace nbh6b

namespace nbl {
// all return a hipError_t as int (0 = launched); one row per lane, grid = ceil(rows / nbd::kLanes) (correct: ceil(m / nbd::kLanes))
// init: base (x0, v0) := the own rows' state, t0 := 0, level := wanted_level(a0, j0); (a0, j0, s0, c0) are the opening's
int launch_hermite6_block_init_kernel(int fp64, hipStream_t stream, const nbh6b::Block6Args& a);
// every own row predicted from its base to b.tau: xp into pos, vp into vel, ap into ap (h_i = (T)(tau - t0_i) * unit,
// coefficients6_of(h_i) per row), and the number of rows that reach tau per tile of kLanes rows into counts
int launch_hermite6_block_predict_kernel(int fp64, hipStream_t stream, const nbh6b::Block6Args& a);
// the rows that reach b.tau, ascending, into active, and their predicted (xp, vp, ap) words and global indices into the query buffers
int launch_hermite6_block_compact_kernel(int fp64, hipStream_t stream, const nbh6b::Block6Args& a);
// the active rows corrected with their own h_i: base := (x1, v1, a1, j1, s1, c1), t0 := tau, pos / vel := (x1, v1), level := next_level
int launch_hermite6_block_correct_kernel(int fp64, hipStream_t stream, const nbh6b::Block6Args& a);
}  // namespace nbl
