// hermite_block.cpp — nbody_step_hermite_block(_d): the Hermite integrator with individual block time steps (include/nbody.h,
// "individual block time steps").  Host C++ only: the scheduler's loop.  Every row carries a tick, a level and its base
// (hermite_block_args.hpp); a sub-step finds tau, the system's smallest next time (one kernel per device and ONE host read: the ranks'
// words through gather_rank_words), predicts every own row to tau into the own slice of pos[cur] and into vel — so the gathers of
// hermite.cpp (hermite_host.hpp) bring the predicted state of ALL bodies to every device and rank as they do for the shared step —,
// and on every device that has a row at tau lists those rows in ascending order with their queries, evaluates them by the jerk POINTS
// pass over queries already on the device (point_sums.cpp: jerk_points_on_device, its split and batches) and corrects them alone.
// A device without an active row takes part in the gathers, which are collective, and launches nothing else.
// The invariant the loop rests on: every t0_i is a multiple of the row's step s_i (a finer level divides it, a coarser one is taken
// only onto an aligned time), so no row steps over a multiple of 2^(levels - 1) ticks and at each such multiple every row is active:
// the last corrector of a call leaves the complete state in pos[cur] / vel.  The base lives in hermite.cpp's buffers of a call
// (he_pos0, he_vel0, he_acc[0], he_jerk[0]; he_acc[1] / he_jerk[1] take the active rows' evaluations), the scheduler's own in hb_*.
// As in hermite.cpp: cur never changes, no force kernel is launched, a call keeps nothing between calls.
#include "hermite_host.hpp"
#include "hermite_block_args.hpp"

#include <cfloat>
#include <cmath>

using namespace nbhb;

namespace nbi {

namespace {

int tiles_of(int rows) { return (rows + nbd::kLanes - 1) / nbd::kLanes; }

}  // namespace

// the scheduler's buffers on every local, and the query buffers of the jerk points pass for as many queries as the local has rows
// (hermite_host.hpp: hermite6_block.cpp takes them too)
int hermite_block_ensure_buffers() {
  const size_t wb = word_bytes();
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    HIPC(hipSetDevice(L.device));
    NBC(L.hb_next.ensure((size_t)g.nranks * sizeof(NextTime)));
    if (L.n_local <= 0) continue;
    const size_t rows = (size_t)L.n_local;
    NBC(L.hb_tick.ensure(rows * sizeof(long long)));
    NBC(L.hb_level.ensure(rows * sizeof(int)));
    NBC(L.hb_counts.ensure((size_t)tiles_of(L.n_local) * sizeof(int)));
    NBC(L.hb_active.ensure(rows * sizeof(int)));
    NBC(L.q_points.ensure(rows * wb));
    NBC(L.q_vel.ensure(rows * wb));
    NBC(L.q_skip.ensure(rows * sizeof(int)));
  }
  return NBODY_OK;
}

namespace {

// what does not change during a call
struct Scheme { int levels; double unit, eta2, lim[kMaxLevels]; };

BlockArgs args_of(Local& L, const Scheme& s, long long tau, int m) {
  BlockArgs a;
  memset(&a, 0, sizeof(a));
  a.pos = word_ptr(L.pos[L.cur], (size_t)L.first);
  a.vel = L.vel;
  a.x0 = L.he_pos0;
  a.v0 = L.he_vel0;
  a.a0 = L.he_acc[0];
  a.j0 = L.he_jerk[0];
  a.a1 = L.he_acc[1];
  a.j1 = L.he_jerk[1];
  a.t0 = L.hb_tick.as<long long>();
  a.level = L.hb_level.as<int>();
  a.counts = L.hb_counts.as<int>();
  a.active = L.hb_active.as<int>();
  a.q_points = L.q_points;
  a.q_vel = L.q_vel;
  a.q_skip = L.q_skip.as<int>();
  a.rows = L.n_local;
  a.first = L.first;
  a.m = m;
  a.levels = s.levels;
  a.tau = tau;
  a.unit = (float)s.unit;
  a.unit_d = s.unit;
  a.eta2 = s.eta2;
  for (int k = 0; k < s.levels; ++k) a.lim[k] = s.lim[k];
  return a;
}

}  // namespace

// tau, the smallest next time over the rows of all ranks, per local the number of its rows that reach it and the system's number
// (the same on every rank): one host read (hermite_host.hpp: hermite6_block.cpp's sub-steps start with it too)
int hermite_block_next_time(int levels, long long* tau, int (&m)[kMaxLocal], long long* active) {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    HIPC(hipSetDevice(L.device));
    HIPC((hipError_t)nbl::launch_hermite_block_next_kernel(L.compute, L.hb_tick.as<long long>(), L.hb_level.as<int>(), std::max(L.n_local, 0),
                                                           levels, L.hb_next.as<NextTime>() + L.rank));
  }
  const NextTime none = {kNoTick, 0, 0};
  std::vector<NextTime> all((size_t)g.nranks, none);
  NBC(gather_rank_words(&Local::hb_next, all.data(), (int)sizeof(NextTime)));
  long long t = kNoTick;
  for (int r = 0; r < g.nranks; ++r)
    if (all[(size_t)r].count > 0) t = std::min(t, all[(size_t)r].tick);
  for (int l = 0; l < g.nlocal; ++l) {
    const NextTime& w = all[(size_t)g.loc[l].rank];
    m[l] = w.count > 0 && w.tick == t ? w.count : 0;
  }
  *active = 0;
  for (int r = 0; r < g.nranks; ++r)
    if (all[(size_t)r].tick == t) *active += all[(size_t)r].count;
  *tau = t;
  return NBODY_OK;
}

namespace {

int one_substep(const Scheme& s, long long tau, const int (&m)[kMaxLocal]) {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC((hipError_t)nbl::launch_hermite_block_predict_kernel(g.fp64, L.compute, args_of(L, s, tau, 0)));
    NBC(hermite_own_slice_written(L));
  }
  NBC(hermite_gather_state());
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (m[l] <= 0) continue;   // no row of this local reaches tau: its predicted slice has travelled, nothing else to do
    HIPC(hipSetDevice(L.device));
    const BlockArgs a = args_of(L, s, tau, m[l]);
    HIPC((hipError_t)nbl::launch_hermite_block_compact_kernel(g.fp64, L.compute, a));
    NBC(jerk_points_on_device(L, m[l], L.he_acc[1], L.he_jerk[1]));
    HIPC((hipError_t)nbl::launch_hermite_block_correct_kernel(g.fp64, L.compute, a));
    NBC(hermite_own_slice_written(L));
  }
  g.steps_done++;
  return NBODY_OK;
}

int step_block_impl(double eta, double dt_max, int levels, int nblocks, long long* substeps, long long* row_evals) {
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
  NBC(hermite_open_call());
  NBC(hermite_block_ensure_buffers());
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC((hipError_t)nbl::launch_hermite_block_init_kernel(g.fp64, L.compute, args_of(L, s, 0, 0)));
  }
  const long long end = (long long)nblocks << (levels - 1);
  long long steps = 0, evals = 0, tau = 0;
  while (tau < end) {
    int m[kMaxLocal] = {0};
    long long active = 0;
    NBC(hermite_block_next_time(s.levels, &tau, m, &active));
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

int nbody_step_hermite_block(float eta, float dt_max, int levels, int nblocks, long long* substeps, long long* row_evals) { NB_ENTER(0);
  return step_block_impl((double)eta, (double)dt_max, levels, nblocks, substeps, row_evals);
}
int nbody_step_hermite_block_d(double eta, double dt_max, int levels, int nblocks, long long* substeps, long long* row_evals) { NB_ENTER(1);
  return step_block_impl(eta, dt_max, levels, nblocks, substeps, row_evals);
}

}  // extern "C"
