// knn.cpp — nbody_knn_rows(_d), nbody_knn(_d): the k nearest bodies and their squared distances, per row or per point the caller
// brings (knn.hip).  Host C++ only.  Flow (query_pass.hpp), exactly the neighbour pass's: reconfigure(), complete_positions() (the
// other slices, as nbody_forces_rows brings them), then per local its rows of the window or its contiguous range of the points:
// upload, the launch (and the combine launch when the sources are split) on the local's compute stream, stream sync, copy back.
// The pass reads pos[cur] and writes only the Local's q_* and kn_* buffers: positions, velocities, arrival counters, partial forces,
// the captured step graph and the force-kernel timer stay as they were.  Nothing outside this file refers to it.
#include "query_pass.hpp"
#include "knn_args.hpp"

using namespace nbq;

namespace nbi {

namespace {

struct Want { bool idx, d2; int k; };

// r.cnt queries on local L — points [r.first, r.first + r.cnt) of the call (uploaded), or with points == null rows
// [r.first, r.first + r.cnt) of L's slice — with the outputs left in kn_idx / kn_d2 ([r.cnt][k]) for the copy back
int launch_knn(Local& L, const void* points, const int* skip, const Range& r, const Want& w) {
  HIPC(hipSetDevice(L.device));
  const size_t wb = word_bytes(), es = elem_bytes(), k = (size_t)w.k;
  if (points) NBC(upload_queries(L, points, skip, r.first, r.cnt));
  if (w.idx) NBC(L.kn_idx.ensure((size_t)r.cnt * k * sizeof(int)));
  if (w.d2) NBC(L.kn_d2.ensure((size_t)r.cnt * k * es));
  const int n_blocks = source_blocks();
  const SplitPlan plan = chunk_split("NBODY_KNN_SPLIT", "NBODY_KNN_SCRATCH_MB", r.cnt, n_blocks, knn_scratch_bytes(1, 1, k, es));
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(knn_scratch_bytes((size_t)plan.batch, (size_t)plan.chunks, k, es)));
  return for_batches(r.cnt, plan, [&](int b0, int m) {
    KnnArgs a;
    memset(&a, 0, sizeof(a));
    fill_sources(a, L, plan, n_blocks, m, points ? 0 : L.first + r.first + b0);
    a.points = points ? L.q_points.as<char>() + (size_t)b0 * wb : nullptr;
    a.skip = points && skip ? L.q_skip.as<int>() + b0 : nullptr;
    a.idx = w.idx ? L.kn_idx.as<int>() + (size_t)b0 * k : nullptr;
    a.d2 = w.d2 ? L.kn_d2.as<char>() + (size_t)b0 * k * es : nullptr;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<void>() : nullptr;
    a.k = w.k;
    HIPC((hipError_t)nbl::launch_knn_kernel(g.fp64, L.compute, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_knn_combine_kernel(g.fp64, L.compute, a));
    return NBODY_OK;
  });
}

// the queries of a call, rows (points == null) or points, over the locals and their results into the caller's arrays
template <typename RangeOf>
int query_impl(RangeOf&& range_of, const void* points, const int* skip, int k, int* idx, void* d2) {
  NBC(reconfigure());
  NBC(complete_positions());
  const Want want = {idx != nullptr, d2 != nullptr, k};
  return run_on_locals(range_of, [&](Local& L, const Range& r) { return launch_knn(L, points, skip, r, want); },
                       [&](Local& L, const Range& r) {
                         NBC(copy_out(idx, r.out, L.kn_idx, r.cnt, (size_t)k * sizeof(int)));
                         return copy_out(d2, r.out, L.kn_d2, r.cnt, (size_t)k * elem_bytes());
                       });
}

bool bad_k(int k) { return k < 1 || k > NBODY_KNN_MAX; }

int rows_impl(int first_row, int n_rows, int k, int* idx, void* d2) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if ((!idx && !d2) || bad_k(k)) return NBODY_ERR_ARG;
  RowWindow w;   // rows as in nbody_forces_rows
  NBC(w.open(first_row, n_rows));
  return query_impl([&](int l) { return rows_of(w, l); }, nullptr, nullptr, k, idx, d2);
}

int points_impl(const void* points, int m, const int* skip, int k, int* idx, void* d2) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!points || m < 1 || (!idx && !d2) || bad_k(k)) return NBODY_ERR_ARG;
  NBC(check_skip(skip, m));
  return query_impl([&](int l) { return points_of(m, l); }, points, skip, k, idx, d2);
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_knn_rows(int first_row, int n_rows, int k, int* idx, float* d2) { NB_ENTER(0);
  return rows_impl(first_row, n_rows, k, idx, d2);
}
int nbody_knn_rows_d(int first_row, int n_rows, int k, int* idx, double* d2) { NB_ENTER(1);
  return rows_impl(first_row, n_rows, k, idx, d2);
}
int nbody_knn(const float* points, int m, const int* skip, int k, int* idx, float* d2) { NB_ENTER(0);
  return points_impl(points, m, skip, k, idx, d2);
}
int nbody_knn_d(const double* points, int m, const int* skip, int k, int* idx, double* d2) { NB_ENTER(1);
  return points_impl(points, m, skip, k, idx, d2);
}

}  // extern "C"
