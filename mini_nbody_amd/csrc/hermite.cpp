// hermite.cpp — nbody_step_hermite(_d), nbody_min_aarseth, nbody_step_hermite_adaptive(_d): the fourth-order Hermite integrator
// (Makino–Aarseth predict, evaluate, correct with a shared dt), the system's smallest |a|^2 / |j|^2 and the shared Aarseth time step
// (include/nbody.h, "fourth-order Hermite integrator").  Host C++ only.  The all-pairs work is the jerk rows pass of point_sums.cpp
// (jerk_own_rows_on_device: its split and batches, no copy back); hermite.hip adds the predictor, the corrector and the reduction.
// A step works in place on the state: the predictor saves the own rows' (x0, v0) in he_pos0 / he_vel0 and writes the predicted rows
// into the own slice of pos[cur] and into vel, so that complete_positions() and gather_velocities() bring the predicted state of ALL
// bodies to every device and rank exactly as they bring the state itself — one device, several devices and nbody_init_rank jobs alike —
// and the jerk pass reads it where it always reads; the corrector then writes the own slice again.  cur never changes, so the captured
// step graph stays valid; the other slices of pos[cur] are marked not present (all_present) and are brought by whoever needs them
// next, as after integrate().  No force kernel is launched: arrival counters, partial forces and the force-kernel timer stay as they
// were.  A call keeps nothing between calls: (a0, j0) is evaluated afresh at its start.  hermite_block.cpp builds on the opening, the
// gathers and the mark of a rewritten slice, hermite6.cpp on the buffers, the gathers, the mark, the minimum and the adaptive loop
// (hermite_host.hpp); nothing else outside this file refers to it.
#include "hermite_host.hpp"
#include "hermite_args.hpp"

#include <cmath>
#include <limits>

using namespace nbh;

namespace nbi {

namespace {

}  // namespace

// the buffers of a call on every local that owns rows, and the ranks' words (hermite_host.hpp: hermite6.cpp takes them too)
int hermite_ensure_buffers() {
  const size_t wb = word_bytes();
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    HIPC(hipSetDevice(L.device));
    NBC(L.he_best.ensure((size_t)g.nranks * sizeof(BestRatio)));
    if (L.n_local <= 0) continue;
    const size_t bytes = (size_t)L.n_local * wb;
    NBC(L.he_pos0.ensure(bytes));
    NBC(L.he_vel0.ensure(bytes));
    for (int k = 0; k < 2; ++k) {
      NBC(L.he_acc[k].ensure(bytes));
      NBC(L.he_jerk[k].ensure(bytes));
    }
  }
  return NBODY_OK;
}

namespace {

// (a, j) of every own row at the state the live buffers hold, into he_acc[k] / he_jerk[k]: the rows form of the jerk pass.  Several
// ranks: the streams are drained before anything travels (a gather writes into the buffer the previous evaluation read), and, with
// several devices in one process, again once the velocities have travelled: gather_velocities() leaves its peer copies OUT of every
// owner's vel on the READERS' compute streams, and the owner's corrector, which writes vel next, is ordered on its own stream behind
// its own jerk pass only.  The drain puts every corrector (and the next predictor) behind every copy; complete_positions() ends in
// the same drain for the positions, and the gather of several processes synchronises by itself.
int evaluate(int k) {
  NBC(hermite_gather_state());
  for (int l = 0; l < g.nlocal; ++l) NBC(jerk_own_rows_on_device(g.loc[l], g.loc[l].he_acc[k], g.loc[l].he_jerk[k]));
  return NBODY_OK;
}

HermiteArgs args_of(Local& L, int k, double h) {
  HermiteArgs a;
  memset(&a, 0, sizeof(a));
  a.pos = word_ptr(L.pos[L.cur], (size_t)L.first);
  a.vel = L.vel;
  a.pos0 = L.he_pos0;
  a.vel0 = L.he_vel0;
  a.a0 = L.he_acc[k];
  a.j0 = L.he_jerk[k];
  a.rows = L.n_local;
  const Coefficients<float> c = coefficients_of((float)h);
  const Coefficients<double> d = coefficients_of(h);
  a.h = c.h; a.c2 = c.c2; a.c3 = c.c3; a.hh = c.hh; a.c12 = c.c12;
  a.h_d = d.h; a.c2_d = d.c2; a.c3_d = d.c3; a.hh_d = d.hh; a.c12_d = d.c12;
  return a;
}

// one step of h (a value of the context precision) from (a0, j0) in he_*[*k]; leaves (a1, j1) in he_*[*k ^ 1] and flips *k
int one_step(double h, int* k) {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC((hipError_t)nbl::launch_hermite_predict_kernel(g.fp64, L.compute, args_of(L, *k, h)));
    NBC(hermite_own_slice_written(L));
  }
  NBC(evaluate(*k ^ 1));
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HermiteArgs a = args_of(L, *k, h);
    a.a1 = L.he_acc[*k ^ 1];
    a.j1 = L.he_jerk[*k ^ 1];
    HIPC((hipError_t)nbl::launch_hermite_correct_kernel(g.fp64, L.compute, a));
    NBC(hermite_own_slice_written(L));
  }
  *k ^= 1;
  g.steps_done++;
  return NBODY_OK;
}

}  // namespace

// the system's smallest q = |a|^2 / |j|^2 over he_acc[k] / he_jerk[k] with the lowest global row that reaches it; +inf and -1 where
// there is none.  The same values on every rank.
int hermite_best_of(int k, double* q, int* row) {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    HIPC(hipSetDevice(L.device));
    HIPC((hipError_t)nbl::launch_hermite_best_kernel(g.fp64, L.compute, L.he_acc[k].as<void>(), L.he_jerk[k].as<void>(), std::max(L.n_local, 0),
                                                     L.first, L.he_best.as<BestRatio>() + L.rank));
  }
  const BestRatio none = {std::numeric_limits<double>::infinity(), -1, 0};
  std::vector<BestRatio> all((size_t)g.nranks, none);
  NBC(gather_rank_words(&Local::he_best, all.data(), (int)sizeof(BestRatio)));
  BestRatio best = none;
  for (int r = 0; r < g.nranks; ++r) {   // rank order = ascending rows: strict < keeps the lowest row
    const BestRatio& b = all[(size_t)r];
    if (b.row >= 0 && b.q < best.q) best = b;
  }
  *q = best.q; *row = best.row;
  return NBODY_OK;
}

namespace {

int step_hermite_impl(double dt, int nsteps) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (nsteps < 1 || !std::isfinite(dt)) return NBODY_ERR_ARG;
  NBC(hermite_open_call());
  int k = 0;
  for (int s = 0; s < nsteps; ++s) NBC(one_step(dt, &k));
  return sync_all();
}

int min_aarseth_impl(double* q, int* row) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!q && !row) return NBODY_ERR_ARG;
  NBC(hermite_open_call());
  double bq = 0.0;
  int br = -1;
  NBC(hermite_best_of(0, &bq, &br));
  if (q) *q = bq;
  if (row) *row = br;
  return NBODY_OK;
}

// The shared Aarseth step (include/nbody.h states the loop).  Everything but the step itself is binary64 on the host; dt is rounded
// once to the context precision, and t advances by the rounded value.  Every rank computes the same h from the same values.
int step_hermite_adaptive_impl(double eta, double t_end, double dt_min, double dt_max, int max_steps, double* t_reached, int* steps_taken) {
  return hermite_adaptive_loop(eta, t_end, dt_min, dt_max, max_steps, t_reached, steps_taken, hermite_open_call, one_step);
}

}  // namespace

// ---- shared with hermite_block.cpp (hermite_host.hpp) ----
int hermite_gather_state() {
  if (g.nranks > 1) NBC(sync_all());
  NBC(complete_positions());
  NBC(gather_velocities());
  if (g.nranks > 1 && !g.multiprocess) NBC(sync_all());
  return NBODY_OK;
}

int hermite_own_slice_written(Local& L) {
  HIPC(hipEventRecord(L.ev_own_ready, L.compute));
  L.all_present = (g.nranks == 1);
  return NBODY_OK;
}

int hermite_open_call() {
  NBC(reconfigure());
  NBC(hermite_ensure_buffers());
  return evaluate(0);
}

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_step_hermite(float dt, int nsteps) { NB_ENTER(0); return step_hermite_impl((double)dt, nsteps); }
int nbody_step_hermite_d(double dt, int nsteps) { NB_ENTER(1); return step_hermite_impl(dt, nsteps); }
int nbody_min_aarseth(double* q, int* row) { NB_REFUSE_WHILE_SERVED(); return min_aarseth_impl(q, row); }
int nbody_step_hermite_adaptive(float eta, float t_end, float dt_min, float dt_max, int max_steps, double* t_reached, int* steps_taken) { NB_ENTER(0);
  return step_hermite_adaptive_impl((double)eta, (double)t_end, (double)dt_min, (double)dt_max, max_steps, t_reached, steps_taken);
}
int nbody_step_hermite_adaptive_d(double eta, double t_end, double dt_min, double dt_max, int max_steps, double* t_reached, int* steps_taken) { NB_ENTER(1);
  return step_hermite_adaptive_impl(eta, t_end, dt_min, dt_max, max_steps, t_reached, steps_taken);
}

}  // extern "C"
