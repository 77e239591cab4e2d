// timescale.cpp — nbody_timescale_rows(_d), nbody_min_timescale(_d), nbody_step_adaptive(_d): per row the smallest pair crossing time
// squared |r_ij|^2 / |v_ij|^2, the body that gives it and the smallest squared distance; the best of the whole system; and a shared
// adaptive time step on top of the existing step (timescale.hip).  Host C++ only, in the shape of neighbors.cpp.  Flow (query_pass.hpp):
// reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings them), all N velocities where every local's
// kernel can read them (query_pass.hpp's gather_velocities), then per local its rows of the window: the launch (and the combine launch when the
// sources are split) on the local's compute stream, stream sync, copy back.  The system form runs the rows pass over every local's own
// rows, reduces them to the local's best on the device and picks the winner among the devices' or ranks' words in rank order on the
// host; processes exchange the words through the transport they use for positions (allgather_rank_words), as the closest pair's.
// The pass reads pos[cur] and vel and writes only the Local's q_scratch, ts_* buffers and (nbody_init_rank contexts) full_scratch:
// positions, velocities, arrival counters, partial forces, the captured step graph and the force-kernel timer stay as they were.
// nbody_step_adaptive is a host loop of the system form and one eager step (step_impl) per pass.  Nothing outside this file refers to it.
#include "query_pass.hpp"
#include "timescale_args.hpp"

#include <cmath>
#include <limits>

using namespace nbts;

namespace nbi {

namespace {

// Workgroups per CU a launch should have before its sources stop being split (query_pass.hpp's choose_chunks), in place of kQueryFill:
// a row's pairs are one dependent chain through the division, and one or two waves a SIMD do not hide it.  Measured on 65 536 rows
// (profiles/r09_timescale.txt): 6.64 ms unsplit, 3.63 ms over the 2 chunks kQueryFill asks for, 3.19 ms over 4, 2.70 ms over 16.
constexpr int kTimescaleFill = 16;

struct Want { bool tau2, idx, d2; };

// rows [r.first, r.first + r.cnt) of L's slice, with the outputs left in ts_tau2 / ts_idx / ts_d2 for the copy back
int launch_timescale(Local& L, const Range& r, const Want& w) {
  HIPC(hipSetDevice(L.device));
  const size_t es = elem_bytes();
  if (w.tau2) NBC(L.ts_tau2.ensure((size_t)r.cnt * es));
  if (w.idx) NBC(L.ts_idx.ensure((size_t)r.cnt * sizeof(int)));
  if (w.d2) NBC(L.ts_d2.ensure((size_t)r.cnt * es));
  const int n_blocks = source_blocks();
  const SplitPlan plan = chunk_split("NBODY_TIMESCALE_SPLIT", "NBODY_TIMESCALE_SCRATCH_MB", r.cnt, n_blocks, timescale_scratch_bytes(1, 1, es),
                                     kTimescaleFill);
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(timescale_scratch_bytes((size_t)plan.batch, (size_t)plan.chunks, es)));
  return for_batches(r.cnt, plan, [&](int b0, int m) {
    TimescaleArgs a;
    memset(&a, 0, sizeof(a));
    fill_sources(a, L, plan, n_blocks, m, L.first + r.first + b0);
    a.vsrc = velocities_of(L);
    a.tau2 = w.tau2 ? L.ts_tau2.as<char>() + (size_t)b0 * es : nullptr;
    a.idx = w.idx ? L.ts_idx.as<int>() + b0 : nullptr;
    a.d2min = w.d2 ? L.ts_d2.as<char>() + (size_t)b0 * es : nullptr;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<void>() : nullptr;
    HIPC((hipError_t)nbl::launch_timescale_kernel(g.fp64, L.compute, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_timescale_combine_kernel(g.fp64, L.compute, a));
    return NBODY_OK;
  });
}

int rows_impl(int first_row, int n_rows, void* tau2, int* idx, void* d2min) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!tau2 && !idx && !d2min) return NBODY_ERR_ARG;
  RowWindow w;   // rows as in nbody_forces_rows
  NBC(w.open(first_row, n_rows));
  NBC(reconfigure());
  NBC(complete_positions());
  NBC(gather_velocities());
  const Want want = {tau2 != nullptr, idx != nullptr, d2min != nullptr};
  return run_on_locals([&](int l) { return rows_of(w, l); }, [&](Local& L, const Range& r) { return launch_timescale(L, r, want); },
                       [&](Local& L, const Range& r) {
                         NBC(copy_out(tau2, r.out, L.ts_tau2, r.cnt, elem_bytes()));
                         NBC(copy_out(idx, r.out, L.ts_idx, r.cnt, sizeof(int)));
                         return copy_out(d2min, r.out, L.ts_d2, r.cnt, elem_bytes());
                       });
}

// the system's smallest tau2 (as fp64: exact in either precision) with the lowest row i that reaches it and i's partner j, and the
// system's smallest d2; -1, -1 and +inf where there is none.  The same values on every rank.
int min_impl(double* tau2, int* i, int* j, double* d2min) {
  NBC(reconfigure());
  NBC(complete_positions());
  NBC(gather_velocities());
  const Want want = {true, true, true};
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local > 0) NBC(launch_timescale(L, {0, L.n_local, 0}, want));
    HIPC(hipSetDevice(L.device));
    NBC(L.ts_best.ensure((size_t)g.nranks * sizeof(BestScale)));
    HIPC((hipError_t)nbl::launch_timescale_best_kernel(g.fp64, L.compute, L.ts_tau2.as<void>(), L.ts_idx.as<int>(), L.ts_d2.as<void>(), L.n_local,
                                                       L.first, L.ts_best.as<BestScale>() + L.rank));
  }
  const double inf = std::numeric_limits<double>::infinity();
  const BestScale none = {inf, inf, -1, -1};
  std::vector<BestScale> all((size_t)g.nranks, none);
  NBC(gather_rank_words(&Local::ts_best, all.data(), (int)sizeof(BestScale)));
  BestScale best = none;
  for (int r = 0; r < g.nranks; ++r) {   // rank order = ascending rows: strict < keeps the lowest i
    const BestScale& b = all[(size_t)r];
    if (b.i >= 0 && b.tau2 < best.tau2) { best.tau2 = b.tau2; best.i = b.i; best.j = b.j; }
    if (b.d2min < best.d2min) best.d2min = b.d2min;
  }
  *tau2 = best.tau2; *i = best.i; *j = best.j; *d2min = best.d2min;
  return NBODY_OK;
}

int min_timescale_impl(double* tau2, int* i, int* j, double* d2min) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!tau2 && !i && !j && !d2min) return NBODY_ERR_ARG;
  double t = 0.0, d = 0.0;
  int bi = -1, bj = -1;
  NBC(min_impl(&t, &bi, &bj, &d));
  if (tau2) *tau2 = t;
  if (i) *i = bi;
  if (j) *j = bj;
  if (d2min) *d2min = d;
  return NBODY_OK;
}

// The shared adaptive step (include/nbody.h states the loop).  Everything but the step itself is binary64 on the host; dt is rounded
// once to the context precision, and t advances by the rounded value.  Every rank computes the same h from the same values.
int step_adaptive_impl(double eta, double t_end, double dt_min, double dt_max, int max_steps, double* t_reached, int* steps_taken) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!std::isfinite(eta) || !std::isfinite(t_end) || !std::isfinite(dt_min) || !std::isfinite(dt_max)) return NBODY_ERR_ARG;
  if (eta <= 0.0 || dt_min <= 0.0 || dt_max < dt_min || t_end <= 0.0 || max_steps < 1) return NBODY_ERR_ARG;
  float eps32;
  memcpy(&eps32, &nbk::kSoftBits, sizeof(eps32));   // the force's eps
  const double eps = (double)eps32;
  double t = 0.0;
  int steps = 0;
  while (t < t_end && steps < max_steps) {
    double tau2, d2min;
    int i, j;
    NBC(min_impl(&tau2, &i, &j, &d2min));
    const double s = d2min + eps;
    const double tff2 = s * std::sqrt(s) / 2.0;   // the unit-mass pair free-fall time squared at the closest pair's distance
    double h = eta * std::sqrt(tau2 < tff2 ? tau2 : tff2);
    h = h > dt_max ? dt_max : h;
    h = h < dt_min ? dt_min : h;
    if (t + h > t_end) h = t_end - t;
    const float dt32 = (float)h;
    const double dt = g.fp64 ? h : (double)dt32;
    NBC(step_impl(g.fp64 ? (float)h : dt32, dt, 1));
    t += dt;
    ++steps;
    if (t_reached) *t_reached = t;
    if (steps_taken) *steps_taken = steps;
  }
  return NBODY_OK;
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_timescale_rows(int first_row, int n_rows, float* tau2, int* idx, float* d2min) { NB_ENTER(0);
  return rows_impl(first_row, n_rows, tau2, idx, d2min);
}
int nbody_timescale_rows_d(int first_row, int n_rows, double* tau2, int* idx, double* d2min) { NB_ENTER(1);
  return rows_impl(first_row, n_rows, tau2, idx, d2min);
}
int nbody_min_timescale(float* tau2, int* i, int* j, float* d2min) { NB_ENTER(0);
  double t = 0.0, d = 0.0;
  NBC(min_timescale_impl(tau2 ? &t : nullptr, i, j, d2min ? &d : nullptr));
  if (tau2) *tau2 = (float)t;     // exact: t and d are binary32 values
  if (d2min) *d2min = (float)d;
  return NBODY_OK;
}
int nbody_min_timescale_d(double* tau2, int* i, int* j, double* d2min) { NB_ENTER(1);
  return min_timescale_impl(tau2, i, j, d2min);
}
int nbody_step_adaptive(float eta, float t_end, float dt_min, float dt_max, int max_steps, double* t_reached, int* steps_taken) { NB_ENTER_UNIT_MASS(0);
  return step_adaptive_impl((double)eta, (double)t_end, (double)dt_min, (double)dt_max, max_steps, t_reached, steps_taken);
}
int nbody_step_adaptive_d(double eta, double t_end, double dt_min, double dt_max, int max_steps, double* t_reached, int* steps_taken) { NB_ENTER_UNIT_MASS(1);
  return step_adaptive_impl(eta, t_end, dt_min, dt_max, max_steps, t_reached, steps_taken);
}

}  // extern "C"
