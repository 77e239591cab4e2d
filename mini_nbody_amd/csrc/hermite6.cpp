// hermite6.cpp — nbody_step_hermite6(_d), nbody_step_hermite6_adaptive(_d): the sixth-order Hermite integrator of Nitadori & Makino
// (2008) with a shared dt (include/nbody.h, "sixth-order Hermite integrator").  Host C++ only.  The all-pairs work is the snap rows pass
// of point_sums.cpp (snap_own_rows_on_device: its split and batches, no copy back); hermite6.hip adds the predictor and the corrector,
// hermite.hip the best-row reduction.
// A step works in place on the state exactly as hermite.cpp's does: the predictor saves the own rows' (x0, v0) in he_pos0 / he_vel0 and
// writes the predicted rows into the own slice of pos[cur] and into vel, so that the gathers bring the predicted state of ALL bodies to
// every device and rank; the predicted accelerations go to h6_ap and travel as the snap call's own accelerations do
// (gather_accelerations).  In an nbody_init_rank job those pass through full_scratch, where the velocities lie afterwards: the
// accelerations are gathered FIRST, the state after them.  cur never changes, so the captured step graph stays valid; no force kernel
// is launched.  A call keeps nothing between calls: (a0, j0, s0) is evaluated afresh at its start — what nbody_snap_rows returns — and
// the crackle starts from zero.  The buffers of the fourth-order step (he_*) serve here too: every call drains its streams before it
// returns, so no two calls use them at once.
#include "hermite_host.hpp"
#include "hermite6_args.hpp"

#include <cmath>

using namespace nbh6;

namespace nbi {

// the buffers of a call on every local that owns rows: hermite.cpp's, and the snap, crackle and predicted-acceleration words
// (hermite_host.hpp: hermite6_block.cpp takes them too)
int hermite6_ensure_buffers() {
  NBC(hermite_ensure_buffers());
  const size_t wb = word_bytes();
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    const size_t bytes = (size_t)L.n_local * wb;
    for (int k = 0; k < 2; ++k) NBC(L.h6_snap[k].ensure(bytes));
    NBC(L.h6_crk.ensure(bytes));
    NBC(L.h6_ap.ensure(bytes));
  }
  return NBODY_OK;
}

namespace {

// (a, j, s) of every own row into he_acc[k] / he_jerk[k] / h6_snap[k] from the sources every device now holds and the N source
// accelerations that lie in `own` on their owners
int snap_rows(int k, DevMem Local::*own) {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    NBC(snap_own_rows_on_device(L, accelerations_of(L, own), L.he_acc[k], L.he_jerk[k], L.h6_snap[k]));
  }
  return NBODY_OK;
}

}  // namespace

// what every call starts with: the configuration, the buffers, (a0, j0, s0) of the state it finds into slot 0 — the two passes of
// nbody_snap_rows — and a crackle of +0 (hermite_host.hpp: hermite6_block.cpp opens with it too)
int hermite6_open_call() {
  NBC(reconfigure());
  NBC(hermite6_ensure_buffers());
  NBC(hermite_gather_state());
  NBC(snap_open_accelerations());
  NBC(snap_rows(0, &Local::sn_acc));
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC(hipMemsetAsync(L.h6_crk, 0, (size_t)L.n_local * word_bytes(), L.compute));
  }
  return NBODY_OK;
}

namespace {

Hermite6Args args_of(Local& L, int k, double h) {
  Hermite6Args a;
  memset(&a, 0, sizeof(a));
  a.pos = word_ptr(L.pos[L.cur], (size_t)L.first);
  a.vel = L.vel;
  a.pos0 = L.he_pos0;
  a.vel0 = L.he_vel0;
  a.a0 = L.he_acc[k];
  a.j0 = L.he_jerk[k];
  a.s0 = L.h6_snap[k];
  a.crk = L.h6_crk;
  a.ap = L.h6_ap;
  a.rows = L.n_local;
  a.f = coefficients6_of((float)h);
  a.d = coefficients6_of(h);
  return a;
}

// one step of h (a value of the context precision) from (a0, j0, s0) in slot *k and c0 in h6_crk; leaves (a1, j1, s1) in slot *k ^ 1,
// c1 in h6_crk and flips *k
int one_step(double h, int* k) {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC((hipError_t)nbl::launch_hermite6_predict_kernel(g.fp64, L.compute, args_of(L, *k, h)));
    NBC(hermite_own_slice_written(L));
  }
  NBC(gather_accelerations(&Local::h6_ap));   // (first: an nbody_init_rank job's velocities end up in full_scratch)
  NBC(hermite_gather_state());
  NBC(snap_rows(*k ^ 1, &Local::h6_ap));
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    Hermite6Args a = args_of(L, *k, h);
    a.a1 = L.he_acc[*k ^ 1];
    a.j1 = L.he_jerk[*k ^ 1];
    a.s1 = L.h6_snap[*k ^ 1];
    HIPC((hipError_t)nbl::launch_hermite6_correct_kernel(g.fp64, L.compute, a));
    NBC(hermite_own_slice_written(L));
  }
  *k ^= 1;
  g.steps_done++;
  return NBODY_OK;
}

int step_hermite6_impl(double dt, int nsteps) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (nsteps < 1 || !std::isfinite(dt)) return NBODY_ERR_ARG;
  NBC(hermite6_open_call());
  int k = 0;
  for (int s = 0; s < nsteps; ++s) NBC(one_step(dt, &k));
  return sync_all();
}

int step_hermite6_adaptive_impl(double eta, double t_end, double dt_min, double dt_max, int max_steps, double* t_reached, int* steps_taken) {
  return hermite_adaptive_loop(eta, t_end, dt_min, dt_max, max_steps, t_reached, steps_taken, hermite6_open_call, one_step);
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_step_hermite6(float dt, int nsteps) { NB_ENTER(0); return step_hermite6_impl((double)dt, nsteps); }
int nbody_step_hermite6_d(double dt, int nsteps) { NB_ENTER(1); return step_hermite6_impl(dt, nsteps); }
int nbody_step_hermite6_adaptive(float eta, float t_end, float dt_min, float dt_max, int max_steps, double* t_reached, int* steps_taken) { NB_ENTER(0);
  return step_hermite6_adaptive_impl((double)eta, (double)t_end, (double)dt_min, (double)dt_max, max_steps, t_reached, steps_taken);
}
int nbody_step_hermite6_adaptive_d(double eta, double t_end, double dt_min, double dt_max, int max_steps, double* t_reached, int* steps_taken) { NB_ENTER(1);
  return step_hermite6_adaptive_impl(eta, t_end, dt_min, dt_max, max_steps, t_reached, steps_taken);
}

}  // extern "C"
