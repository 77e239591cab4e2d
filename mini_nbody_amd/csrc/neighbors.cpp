// neighbors.cpp — nbody_neighbors_rows(_d), nbody_nearest(_d), nbody_closest_pair(_d): the nearest body, its squared distance and the
// number of bodies within a radius, per row or per point the caller brings, and the closest pair of the system (neighbors.hip).  Host
// C++ only.  Flow (query_pass.hpp): reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings them), then per
// local its rows of the window or its contiguous range of the points: upload, the launch (and the combine launch when the sources are
// split) on the local's compute stream, stream sync, copy back.  The closest pair runs the rows pass over every local's own rows,
// reduces them to the local's best row on the device and picks the winner among the devices' or ranks' triples in rank order on the
// host; processes exchange the triples through the transport they use for positions (allgather_rank_words), as the energy totals.
// The pass reads pos[cur] and writes only the Local's q_* and nb_* buffers: positions, velocities, arrival counters, partial forces,
// the captured step graph and the force-kernel timer stay as they were.  Nothing outside this file refers to it.
#include "query_pass.hpp"
#include "neighbors_args.hpp"

#include <limits>

using namespace nbn;

namespace nbi {

namespace {

// the hot loop's form when NBODY_NEIGHBORS_LOOP does not say
constexpr int kNbDefaultLoop = kNbLoopWindow;

struct Want { bool idx, d2, count; double r2; };

// r.cnt queries on local L — points [r.first, r.first + r.cnt) of the call (uploaded), or with points == null rows
// [r.first, r.first + r.cnt) of L's slice — with the outputs left in nb_idx / nb_d2 / nb_count for the copy back
int launch_neighbors(Local& L, const void* points, const int* skip, const Range& r, const Want& w) {
  HIPC(hipSetDevice(L.device));
  const size_t wb = word_bytes(), es = elem_bytes();
  if (points) NBC(upload_queries(L, points, skip, r.first, r.cnt));
  if (w.idx) NBC(L.nb_idx.ensure((size_t)r.cnt * sizeof(int)));
  if (w.d2) NBC(L.nb_d2.ensure((size_t)r.cnt * es));
  if (w.count) NBC(L.nb_count.ensure((size_t)r.cnt * sizeof(int)));
  const int n_blocks = source_blocks();
  const long long asked_loop = env_ll("NBODY_NEIGHBORS_LOOP", 0);   // 1: the scan, 2: the window form (same results), else the default
  const int loop = asked_loop == kNbLoopScan || asked_loop == kNbLoopWindow ? (int)asked_loop : kNbDefaultLoop;
  const SplitPlan plan = chunk_split("NBODY_NEIGHBORS_SPLIT", "NBODY_NEIGHBORS_SCRATCH_MB", r.cnt, n_blocks, neighbors_scratch_bytes(1, 1, es));
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(neighbors_scratch_bytes((size_t)plan.batch, (size_t)plan.chunks, es)));
  return for_batches(r.cnt, plan, [&](int b0, int m) {
    NeighborsArgs a;
    memset(&a, 0, sizeof(a));
    fill_sources(a, L, plan, n_blocks, m, points ? 0 : L.first + r.first + b0);
    a.points = points ? L.q_points.as<char>() + (size_t)b0 * wb : nullptr;
    a.skip = points && skip ? L.q_skip.as<int>() + b0 : nullptr;
    a.idx = w.idx ? L.nb_idx.as<int>() + b0 : nullptr;
    a.d2 = w.d2 ? L.nb_d2.as<char>() + (size_t)b0 * es : nullptr;
    a.count = w.count ? L.nb_count.as<int>() + b0 : nullptr;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<void>() : nullptr;
    a.r2 = w.count ? w.r2 : 0.0;
    HIPC((hipError_t)nbl::launch_neighbors_kernel(g.fp64, loop, L.compute, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_neighbors_combine_kernel(g.fp64, L.compute, a));
    return NBODY_OK;
  });
}

// the queries of a call, rows (points == null) or points, over the locals and their results into the caller's arrays
template <typename RangeOf>
int query_impl(RangeOf&& range_of, const void* points, const int* skip, int* idx, void* d2, double r2, int* count) {
  NBC(reconfigure());
  NBC(complete_positions());
  const Want want = {idx != nullptr, d2 != nullptr, count != nullptr, r2};
  return run_on_locals(range_of, [&](Local& L, const Range& r) { return launch_neighbors(L, points, skip, r, want); },
                       [&](Local& L, const Range& r) {
                         NBC(copy_out(idx, r.out, L.nb_idx, r.cnt, sizeof(int)));
                         NBC(copy_out(d2, r.out, L.nb_d2, r.cnt, elem_bytes()));
                         return copy_out(count, r.out, L.nb_count, r.cnt, sizeof(int));
                       });
}

int rows_impl(int first_row, int n_rows, int* idx, void* d2, double r2, int* count) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!idx && !d2 && !count) return NBODY_ERR_ARG;
  RowWindow w;   // rows as in nbody_forces_rows
  NBC(w.open(first_row, n_rows));
  return query_impl([&](int l) { return rows_of(w, l); }, nullptr, nullptr, idx, d2, r2, count);
}

int nearest_impl(const void* points, int m, const int* skip, int* idx, void* d2, double r2, int* count) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!points || m < 1 || (!idx && !d2 && !count)) return NBODY_ERR_ARG;
  NBC(check_skip(skip, m));
  return query_impl([&](int l) { return points_of(m, l); }, points, skip, idx, d2, r2, count);
}

// *i < *j of the smallest d2 (as fp64: exact in either precision); -1, -1, +inf when there is no pair
int closest_pair_impl(int* i, int* j, double* d2) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!i && !j && !d2) return NBODY_ERR_ARG;
  NBC(reconfigure());
  NBC(complete_positions());
  const Want want = {true, true, false, 0.0};
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local > 0) NBC(launch_neighbors(L, nullptr, nullptr, {0, L.n_local, 0}, want));
    HIPC(hipSetDevice(L.device));
    NBC(L.nb_best.ensure((size_t)g.nranks * sizeof(BestPair)));
    HIPC((hipError_t)nbl::launch_neighbors_best_kernel(g.fp64, L.compute, L.nb_d2.as<void>(), L.nb_idx.as<int>(), L.n_local, L.first,
                                                       L.nb_best.as<BestPair>() + L.rank));
  }
  const BestPair none = {std::numeric_limits<double>::infinity(), -1, -1};
  std::vector<BestPair> all((size_t)g.nranks, none);
  NBC(gather_rank_words(&Local::nb_best, all.data(), (int)sizeof(BestPair)));
  BestPair best = none;
  for (int r = 0; r < g.nranks; ++r)   // rank order = ascending rows: strict < keeps the lowest i
    if (all[(size_t)r].i >= 0 && all[(size_t)r].d2 < best.d2) best = all[(size_t)r];
  if (i) *i = best.i;
  if (j) *j = best.j;
  if (d2) *d2 = best.d2;
  return NBODY_OK;
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_neighbors_rows(int first_row, int n_rows, int* idx, float* d2, float r2, int* count) { NB_ENTER(0);
  return rows_impl(first_row, n_rows, idx, d2, (double)r2, count);
}
int nbody_neighbors_rows_d(int first_row, int n_rows, int* idx, double* d2, double r2, int* count) { NB_ENTER(1);
  return rows_impl(first_row, n_rows, idx, d2, r2, count);
}
int nbody_nearest(const float* points, int m, const int* skip, int* idx, float* d2, float r2, int* count) { NB_ENTER(0);
  return nearest_impl(points, m, skip, idx, d2, (double)r2, count);
}
int nbody_nearest_d(const double* points, int m, const int* skip, int* idx, double* d2, double r2, int* count) { NB_ENTER(1);
  return nearest_impl(points, m, skip, idx, d2, r2, count);
}
int nbody_closest_pair(int* i, int* j, float* d2) { NB_ENTER(0);
  double v = 0.0;
  NBC(closest_pair_impl(i, j, i || j || d2 ? &v : nullptr));
  if (d2) *d2 = (float)v;   // exact: v is a binary32 value
  return NBODY_OK;
}
int nbody_closest_pair_d(int* i, int* j, double* d2) { NB_ENTER(1);
  return closest_pair_impl(i, j, d2);
}

}  // extern "C"
