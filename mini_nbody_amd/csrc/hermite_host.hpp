// hermite_host.hpp — what hermite.cpp shares with hermite_block.cpp, hermite6.cpp and hermite6_block.cpp (host C++ only): the opening of a Hermite call,
// its buffers, the gathers that bring the predicted state of all bodies to every device and rank, the mark of a rewritten own slice,
// the system's smallest |a|^2 / |j|^2 and the shared Aarseth loop.  hermite.cpp defines them; none refers to a device symbol beyond those
// of hermite.hip and point_sums.hip.  Two are hermite_block.cpp's (the scheduler's buffers and the next-time read; device symbol: the next-time
// launch of hermite_block.hip) and two hermite6.cpp's (the sixth-order call's buffers and its opening; no device symbol beyond those of
// point_sums.hip): hermite6_block.cpp builds on the four.
#pragma once
#include "query_pass.hpp"

#include <cmath>

namespace nbi {

// what every Hermite call starts with: the configuration, the buffers of a call (he_*), (a0, j0) of the state it finds into he_*[0]
int hermite_open_call();
// The live buffers' own slices have been rewritten (a predictor): positions and velocities of ALL bodies to every device and rank,
// with the drains an evaluation needs before and after (hermite.cpp says why); what follows is a jerk pass on every local
int hermite_gather_state();
// the own slice of pos[cur] has been rewritten on L's compute stream: what the next gather waits for
int hermite_own_slice_written(Local& L);
// the buffers of a call (he_*) on every local that owns rows, and the ranks' words
int hermite_ensure_buffers();
// the system's smallest q = |a|^2 / |j|^2 over he_acc[k] / he_jerk[k] with the lowest global row that reaches it; +inf and -1 where
// there is none.  The same values on every rank
int hermite_best_of(int k, double* q, int* row);

// ---- hermite_block.cpp ----
// the block scheduler's buffers (hb_*) on every local, and q_points, q_vel, q_skip for as many queries as the local has rows
int hermite_block_ensure_buffers();
// tau, the smallest next time t0_i + s_i over the rows of all ranks (hb_tick, hb_level; `levels` levels), m[l] the rows of local l that
// reach it and *active the system's number, the same on every rank: one kernel per local and ONE host read
int hermite_block_next_time(int levels, long long* tau, int (&m)[kMaxLocal], long long* active);

// ---- hermite6.cpp ----
// the buffers of a sixth-order call on every local that owns rows: those above and h6_snap, h6_crk, h6_ap
int hermite6_ensure_buffers();
// what every sixth-order call starts with: the configuration, the buffers, (a0, j0, s0) of the state it finds into he_acc[0], he_jerk[0],
// h6_snap[0] — the two passes of nbody_snap_rows — and a crackle of +0 in h6_crk; the launches are left on the compute streams
int hermite6_open_call();

// The shared Aarseth step (include/nbody.h states the loop) over an integrator's opening, open(), and its step, step(dt, &k), which
// leaves the carried (a, j) in he_acc[k] / he_jerk[k].  Everything but the step itself is binary64 on the host; dt is rounded once to
// the context precision, and t advances by the rounded value.  Every rank computes the same h from the same values.
template <typename Open, typename Step>
int hermite_adaptive_loop(double eta, double t_end, double dt_min, double dt_max, int max_steps, double* t_reached, int* steps_taken,
                          Open&& open, Step&& step) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!std::isfinite(eta) || !std::isfinite(t_end) || !std::isfinite(dt_min) || !std::isfinite(dt_max)) return NBODY_ERR_ARG;
  if (eta <= 0.0 || dt_min <= 0.0 || dt_max < dt_min || t_end <= 0.0 || max_steps < 1) return NBODY_ERR_ARG;
  NBC(open());
  double t = 0.0;
  int steps = 0, k = 0;
  while (t < t_end && steps < max_steps) {
    double q;
    int row;
    NBC(hermite_best_of(k, &q, &row));
    double h = eta * std::sqrt(q);
    h = h > dt_max ? dt_max : h;
    h = h < dt_min ? dt_min : h;
    if (t + h > t_end) h = t_end - t;
    const double dt = g.fp64 ? h : (double)(float)h;
    NBC(step(dt, &k));
    t += dt;
    ++steps;
    if (t_reached) *t_reached = t;
    if (steps_taken) *steps_taken = steps;
  }
  return sync_all();
}

}  // namespace nbi
