// neighbors.cpp — nbody_neighbors_rows(_d), nbody_nearest(_d), nbody_closest_pair(_d): the nearest body, its squared distance and the
// number of bodies within a radius, per row or per point the caller brings, and the closest pair of the system (neighbors.hip).  Host
// C++ only.  Flow, as field.cpp's: reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings them), then per
// local its rows of the window or its contiguous range of the points: upload, the launch (and the combine launch when the sources are
// split) on the local's compute stream, stream sync, copy back.  The closest pair runs the rows pass over every local's own rows,
// reduces them to the local's best row on the device and picks the winner among the devices' or ranks' triples in rank order on the
// host; processes exchange the triples through the transport they use for positions (allgather_rank_words), as the energy totals.
// The pass reads pos[cur] and writes only the Local's nb_* buffers: positions, velocities, arrival counters, partial forces, the
// captured step graph and the force-kernel timer stay as they were.  Nothing outside this file refers to it.
#include "nbody_internal.hpp"
#include "neighbors_args.hpp"

#include <limits>

using namespace nbn;

namespace nbi {

namespace {

// Workgroups the launch should have before the sources stop being split, in units of the CU count (field.cpp's choose_chunks)
constexpr int kNbFill = 2;
// the hot loop's form when NBODY_NEIGHBORS_LOOP does not say
constexpr int kNbDefaultLoop = kNbLoopWindow;

long long env_ll(const char* name, long long dflt) {
  const char* e = getenv(name);
  return e && *e ? atoll(e) : dflt;
}

// C, the number of source chunks (grid.y) of a launch of `queries` queries over n_blocks blocks.  forced >= 1
// (NBODY_NEIGHBORS_SPLIT): min(forced, n_blocks).  Auto: 1 when the queries alone give kNbFill workgroups per CU, else the smallest
// number of chunks that does.
int choose_chunks(long long forced, int queries, int n_blocks) {
  if (forced >= 1) return (int)std::min<long long>(forced, n_blocks);
  const long long groups = ((long long)queries + kNbQueries - 1) / kNbQueries;
  const long long want = (long long)kNbFill * std::max(1, g.cu_count);
  if (groups >= want) return 1;
  return (int)std::min<long long>((want + groups - 1) / groups, n_blocks);
}

struct Want { bool idx, d2, count; double r2; };

// cnt queries on local L — points [p0, p0 + cnt) of the call (uploaded), or with points == null rows [p0, p0 + cnt) of L's slice —
// with the outputs left in nb_idx / nb_d2 / nb_count for the copy back
int launch_neighbors(Local& L, const void* points, const int* skip, int p0, int cnt, const Want& w) {
  HIPC(hipSetDevice(L.device));
  const size_t wb = word_bytes(), es = g.fp64 ? sizeof(double) : sizeof(float);
  if (points) {
    NBC(L.nb_points.ensure((size_t)cnt * wb));
    HIPC(hipMemcpy(L.nb_points, (const char*)points + (size_t)p0 * wb, (size_t)cnt * wb, hipMemcpyHostToDevice));
    if (skip) {
      NBC(L.nb_skip.ensure((size_t)cnt * sizeof(int)));
      HIPC(hipMemcpy(L.nb_skip, skip + p0, (size_t)cnt * sizeof(int), hipMemcpyHostToDevice));
    }
  }
  if (w.idx) NBC(L.nb_idx.ensure((size_t)cnt * sizeof(int)));
  if (w.d2) NBC(L.nb_d2.ensure((size_t)cnt * es));
  if (w.count) NBC(L.nb_count.ensure((size_t)cnt * sizeof(int)));

  const int n_blocks = (g.n + kNbBlock - 1) / kNbBlock;
  const long long forced = env_ll("NBODY_NEIGHBORS_SPLIT", 0);
  const char* mb = getenv("NBODY_NEIGHBORS_SCRATCH_MB");
  const double bound = std::max(0.0, mb && *mb ? atof(mb) : 256.0) * 1048576.0;
  const long long asked_loop = env_ll("NBODY_NEIGHBORS_LOOP", 0);   // 1: the scan, 2: the window form (same results), else the default
  const int loop = asked_loop == kNbLoopScan || asked_loop == kNbLoopWindow ? (int)asked_loop : kNbDefaultLoop;
  // the chunks are chosen from the call's queries; the queries whose chunk results fit the scratch bound go together, in whole workgroups
  int chunk_blocks = n_blocks, chunks = 1, batch = cnt;
  const int asked = choose_chunks(forced, cnt, n_blocks);
  if (asked > 1) {
    chunk_blocks = (n_blocks + asked - 1) / asked;
    chunks = (n_blocks + chunk_blocks - 1) / chunk_blocks;   // no empty chunk
    const double fit = bound / (double)neighbors_scratch_bytes(1, (size_t)chunks, es);
    if (fit < (double)cnt) batch = (int)fit / kNbQueries * kNbQueries;
    if (batch <= 0) { chunk_blocks = n_blocks; chunks = 1; batch = cnt; }   // not one workgroup's queries fit: no split
  }
  if (chunks > 1) NBC(L.nb_scratch.ensure(neighbors_scratch_bytes((size_t)batch, (size_t)chunks, es)));

  for (int b0 = 0; b0 < cnt; b0 += batch) {
    NeighborsArgs a;
    memset(&a, 0, sizeof(a));
    a.src = L.pos[L.cur];
    a.points = points ? L.nb_points.as<char>() + (size_t)b0 * wb : nullptr;
    a.skip = points && skip ? L.nb_skip.as<int>() + b0 : nullptr;
    a.idx = w.idx ? L.nb_idx.as<int>() + b0 : nullptr;
    a.d2 = w.d2 ? L.nb_d2.as<char>() + (size_t)b0 * es : nullptr;
    a.count = w.count ? L.nb_count.as<int>() + b0 : nullptr;
    a.scratch = chunks > 1 ? L.nb_scratch.as<void>() : nullptr;
    a.r2 = w.count ? w.r2 : 0.0;
    a.n_src = g.n;
    a.m = std::min(batch, cnt - b0);
    a.first = points ? 0 : L.first + p0 + b0;
    a.n_blocks = n_blocks;
    a.chunk_blocks = chunk_blocks;
    a.chunks = chunks;
    HIPC((hipError_t)nbl::launch_neighbors_kernel(g.fp64, loop, L.compute, a));
    if (chunks > 1) HIPC((hipError_t)nbl::launch_neighbors_combine_kernel(g.fp64, L.compute, a));
  }
  return NBODY_OK;
}

// after the local's stream is drained: cnt results into the caller's arrays from element `at`
int copy_back(Local& L, int at, int cnt, int* idx, void* d2, int* count) {
  const size_t es = g.fp64 ? sizeof(double) : sizeof(float);
  HIPC(hipSetDevice(L.device));
  HIPC(hipStreamSynchronize(L.compute));   // then blocking copies into the caller's pageable memory, as the other entry points do
  if (idx) HIPC(hipMemcpy(idx + at, L.nb_idx, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost));
  if (d2) HIPC(hipMemcpy((char*)d2 + (size_t)at * es, L.nb_d2, (size_t)cnt * es, hipMemcpyDeviceToHost));
  if (count) HIPC(hipMemcpy(count + at, L.nb_count, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost));
  return NBODY_OK;
}

int rows_impl(int first_row, int n_rows, int* idx, void* d2, double r2, int* count) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!idx && !d2 && !count) return NBODY_ERR_ARG;
  RowWindow w;   // rows as in nbody_forces_rows
  NBC(w.open(first_row, n_rows));
  NBC(reconfigure());
  NBC(complete_positions());
  const Want want = {idx != nullptr, d2 != nullptr, count != nullptr, r2};
  for (int l = 0; l < g.nlocal; ++l) {
    int r0, cnt;
    if (w.rows_of(g.loc[l], &r0, &cnt)) NBC(launch_neighbors(g.loc[l], nullptr, nullptr, r0, cnt, want));
  }
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    int r0, cnt;
    if (w.rows_of(L, &r0, &cnt)) NBC(copy_back(L, L.first + r0 - w.g0, cnt, idx, d2, count));
  }
  return NBODY_OK;
}

int nearest_impl(const void* points, int m, const int* skip, int* idx, void* d2, double r2, int* count) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!points || m < 1 || (!idx && !d2 && !count)) return NBODY_ERR_ARG;
  if (skip)
    for (int p = 0; p < m; ++p)
      if (skip[p] < -1 || skip[p] >= g.n) return NBODY_ERR_ARG;
  NBC(reconfigure());
  NBC(complete_positions());
  const Want want = {idx != nullptr, d2 != nullptr, count != nullptr, r2};
  // the points in contiguous ranges over the locals, as the field pass divides them
  auto first_of = [&](int l) { return (int)((long long)m * l / g.nlocal); };
  for (int l = 0; l < g.nlocal; ++l) {
    const int p0 = first_of(l), cnt = first_of(l + 1) - p0;
    if (cnt > 0) NBC(launch_neighbors(g.loc[l], points, skip, p0, cnt, want));
  }
  for (int l = 0; l < g.nlocal; ++l) {
    const int p0 = first_of(l), cnt = first_of(l + 1) - p0;
    if (cnt > 0) NBC(copy_back(g.loc[l], p0, cnt, idx, d2, count));
  }
  return NBODY_OK;
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
    if (L.n_local > 0) NBC(launch_neighbors(L, nullptr, nullptr, 0, L.n_local, want));
    HIPC(hipSetDevice(L.device));
    NBC(L.nb_best.ensure((size_t)g.nranks * sizeof(BestPair)));
    HIPC((hipError_t)nbl::launch_neighbors_best_kernel(g.fp64, L.compute, L.nb_d2.as<void>(), L.nb_idx.as<int>(), L.n_local, L.first,
                                                       L.nb_best.as<BestPair>() + L.rank));
  }
  const BestPair none = {std::numeric_limits<double>::infinity(), -1, -1};
  std::vector<BestPair> all((size_t)g.nranks, none);
  if (g.multiprocess && g.nranks > 1) {
    Local& L = g.loc[0];
    NBC(allgather_rank_words(L, L.nb_best, all.data(), (int)sizeof(BestPair)));
  } else {
    for (int l = 0; l < g.nlocal; ++l) {
      Local& L = g.loc[l];
      HIPC(hipSetDevice(L.device));
      HIPC(hipStreamSynchronize(L.compute));
      HIPC(hipMemcpy(&all[(size_t)L.rank], L.nb_best.as<BestPair>() + L.rank, sizeof(BestPair), hipMemcpyDeviceToHost));
    }
  }
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

int nbody_neighbors_rows(int first_row, int n_rows, int* idx, float* d2, float r2, int* count) { NB_REFUSE_WHILE_SERVED();
  if (g.init && g.fp64) return NBODY_ERR_STATE;
  return rows_impl(first_row, n_rows, idx, d2, (double)r2, count);
}
int nbody_neighbors_rows_d(int first_row, int n_rows, int* idx, double* d2, double r2, int* count) { NB_REFUSE_WHILE_SERVED();
  if (g.init && !g.fp64) return NBODY_ERR_STATE;
  return rows_impl(first_row, n_rows, idx, d2, r2, count);
}
int nbody_nearest(const float* points, int m, const int* skip, int* idx, float* d2, float r2, int* count) { NB_REFUSE_WHILE_SERVED();
  if (g.init && g.fp64) return NBODY_ERR_STATE;
  return nearest_impl(points, m, skip, idx, d2, (double)r2, count);
}
int nbody_nearest_d(const double* points, int m, const int* skip, int* idx, double* d2, double r2, int* count) { NB_REFUSE_WHILE_SERVED();
  if (g.init && !g.fp64) return NBODY_ERR_STATE;
  return nearest_impl(points, m, skip, idx, d2, r2, count);
}
int nbody_closest_pair(int* i, int* j, float* d2) { NB_REFUSE_WHILE_SERVED();
  if (g.init && g.fp64) return NBODY_ERR_STATE;
  double v = 0.0;
  NBC(closest_pair_impl(i, j, i || j || d2 ? &v : nullptr));
  if (d2) *d2 = (float)v;   // exact: v is a binary32 value
  return NBODY_OK;
}
int nbody_closest_pair_d(int* i, int* j, double* d2) { NB_REFUSE_WHILE_SERVED();
  if (g.init && !g.fp64) return NBODY_ERR_STATE;
  return closest_pair_impl(i, j, d2);
}

}  // extern "C"
