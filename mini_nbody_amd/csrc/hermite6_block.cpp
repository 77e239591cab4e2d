// hermite6_block.cpp — nbody_step_hermite6_block(_d): the sixth-order Hermite integrator with individual block time steps
// (include/nbody.h, "sixth-order individual block time steps"): the join of hermite6.cpp's scheme and hermite_block.cpp's scheduler.
// Host C++ only: the scheduler's loop.  Every row carries a tick, a level and its base (hermite6_block_args.hpp); a call opens as
// nbody_step_hermite6 does (hermite6.cpp's opening: (a0, j0, s0) from the two passes of nbody_snap_rows, c0 = +0), a sub-step finds tau
// as hermite_block.cpp's does (its next-time read: ONE host read), predicts every own row to tau — xp into the own slice of pos[cur],
// vp into vel, ap into h6_ap —, gathers the predicted accelerations FIRST and the state after them (an nbody_init_rank job's
// accelerations pass through full_scratch, where the velocities lie afterwards; hermite6.cpp says the same), and on every device that
// has a row at tau lists those rows in ascending order with their queries, evaluates them by the snap POINTS pass over queries already
// on the device (point_sums.cpp: snap_points_on_device, its split and batches) and corrects them alone.  A device without an active
// row takes part in the gathers, which are collective, and launches nothing else.  The level rule is the fourth-order scheduler's, on
// |a|^2 / |j|^2, and so is the invariant the loop rests on (hermite_block.cpp states it): at every multiple of 2^(levels - 1) ticks
// every row is active, and the last corrector of a call leaves the complete state in pos[cur] / vel.
// The base lives in the buffers of a sixth-order call (he_pos0, he_vel0, he_acc[0], he_jerk[0], h6_snap[0], h6_crk); he_acc[1],
// he_jerk[1] and h6_snap[1] take the active rows' evaluations, the scheduler's own words are hb_*, the queries q_points, q_vel, q_acc
// and q_skip.  As in hermite6.cpp: cur never changes, no force kernel is launched, a call keeps nothing between calls and drains its
// streams before it returns.  The only host file that names the launch functions of hermite6_block.hip.
#include "hermite_host.hpp"
#include "hermite6_block_args.hpp"

#include <cfloat>
#include <cmath>

using namespace nbhb;
using namespace nbh6b;

namespace nbi {

namespace {

// the query buffer of the snap points pass that the fourth-order scheduler does not need: as many acceleration words as the local has rows
int ensure_query_accelerations() {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    NBC(L.q_acc.ensure((size_t)L.n_local * word_bytes()));
  }
  return NBODY_OK;
}

// what does not change during a call
struct Scheme { int levels; double unit, eta2, lim[kMaxLevels]; };

Block6Args args_of(Local& L, const Scheme& s, long long tau, int m) {
  Block6Args a;
  memset(&a, 0, sizeof(a));
  a.b.pos = word_ptr(L.pos[L.cur], (size_t)L.first);
  a.b.vel = L.vel;
  a.b.x0 = L.he_pos0;
  a.b.v0 = L.he_vel0;
  a.b.a0 = L.he_acc[0];
  a.b.j0 = L.he_jerk[0];
  a.s0 = L.h6_snap[0];
  a.c0 = L.h6_crk;
  a.ap = L.h6_ap;
  a.b.a1 = L.he_acc[1];
  a.b.j1 = L.he_jerk[1];
  a.s1 = L.h6_snap[1];
  a.b.t0 = L.hb_tick.as<long long>();
  a.b.level = L.hb_level.as<int>();
  a.b.counts = L.hb_counts.as<int>();
  a.b.active = L.hb_active.as<int>();
  a.b.q_points = L.q_points;
  a.b.q_vel = L.q_vel;
  a.q_acc = L.q_acc;
  a.b.q_skip = L.q_skip.as<int>();
  a.b.rows = L.n_local;
  a.b.first = L.first;
  a.b.m = m;
  a.b.levels = s.levels;
  a.b.tau = tau;
  a.b.unit = (float)s.unit;
  a.b.unit_d = s.unit;
  a.b.eta2 = s.eta2;
  for (int k = 0; k < s.levels; ++k) a.b.lim[k] = s.lim[k];
  return a;
}

int one_substep(const Scheme& s, long long tau, const int (&m)[kMaxLocal]) {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC((hipError_t)nbl::launch_hermite6_block_predict_kernel(g.fp64, L.compute, args_of(L, s, tau, 0)));
    NBC(hermite_own_slice_written(L));
  }
  NBC(gather_accelerations(&Local::h6_ap));   // (first: an nbody_init_rank job's velocities end up in full_scratch)
  NBC(hermite_gather_state());
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (m[l] <= 0) continue;   // no row of this local reaches tau: its predicted slice has travelled, nothing else to do
    HIPC(hipSetDevice(L.device));
    const Block6Args a = args_of(L, s, tau, m[l]);
    HIPC((hipError_t)nbl::launch_hermite6_block_compact_kernel(g.fp64, L.compute, a));
    NBC(snap_points_on_device(L, m[l], accelerations_of(L, &Local::h6_ap), L.he_acc[1], L.he_jerk[1], L.h6_snap[1]));
    HIPC((hipError_t)nbl::launch_hermite6_block_correct_kernel(g.fp64, L.compute, a));
    NBC(hermite_own_slice_written(L));
  }
  g.steps_done++;
  return NBODY_OK;
}

int step_block6_impl(double eta, double dt_max, int levels, int nblocks, long long* substeps, long long* row_evals) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!std::isfinite(eta) || !std::isfinite(dt_max) || eta <= 0.0 || dt_max <= 0.0) return NBODY_ERR_ARG;
  if (levels < 1 || levels > kMaxLevels || nblocks < 1) return NBODY_ERR_ARG;
  Scheme s;
  s.levels = levels;
  s.unit = std::ldexp(dt_max, -(levels - 1));   // an exact scaling of a T value once it is normal in T
  if (s.unit < (g.fp64 ? DBL_MIN : (double)FLT_MIN)) return NBODY_ERR_ARG;
  s.eta2 = eta * eta;
  for (int k = 0; k < levels; ++k) {
    const double dk = std::ldexp(dt_max, -k);
    s.lim[k] = dk * dk;
  }
  NBC(hermite6_open_call());
  NBC(hermite_block_ensure_buffers());
  NBC(ensure_query_accelerations());
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC((hipError_t)nbl::launch_hermite6_block_init_kernel(g.fp64, L.compute, args_of(L, s, 0, 0)));
  }
  const long long end = (long long)nblocks << (levels - 1);
  long long steps = 0, evals = 0, tau = 0;
  while (tau < end) {
    int m[kMaxLocal] = {0};
    long long active = 0;
    NBC(hermite_block_next_time(levels, &tau, m, &active));
    if (tau > end) return NBODY_ERR_STATE;   // (the invariant: a step never crosses a multiple of 2^(levels - 1))
    NBC(one_substep(s, tau, m));
    ++steps;
    evals += active;
    if (substeps) *substeps = steps;
    if (row_evals) *row_evals = evals;
  }
  return sync_all();
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_step_hermite6_block(float eta, float dt_max, int levels, int nblocks, long long* substeps, long long* row_evals) { NB_ENTER(0);
  return step_block6_impl((double)eta, (double)dt_max, levels, nblocks, substeps, row_evals);
}
int nbody_step_hermite6_block_d(double eta, double dt_max, int levels, int nblocks, long long* substeps, long long* row_evals) { NB_ENTER(1);
  return step_block6_impl(eta, dt_max, levels, nblocks, substeps, row_evals);
}

}  // extern "C"
