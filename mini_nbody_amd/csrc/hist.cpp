// hist.cpp — nbody_radial_counts_rows(_d), nbody_radial_counts(_d), nbody_pair_histogram(_d): the number of bodies in each shell of
// squared distance, per row or per point the caller brings, and the pair counts of the whole system (hist.hip).  Host C++ only.  Flow
// (query_pass.hpp), exactly the neighbour pass's: the edges validated in the context precision, reconfigure(), complete_positions()
// (the other slices, as nbody_forces_rows brings them), then per local its rows of the window or its contiguous range of the points:
// upload, the launch (and the combine launch when the sources are split) on the local's compute stream, stream sync, copy back.  The
// pair histogram runs the rows pass over every local's own rows in batches, adds each batch on the device into the local's 64-bit sums
// (the per-row counts never reach the host) and adds the devices' or ranks' sums in rank order on the host; processes exchange the
// sums through the transport they use for positions (allgather_rank_words), as the closest pair's triples.
// The pass reads pos[cur] and writes only the Local's q_* and hi_* buffers: positions, velocities, arrival counters, partial forces,
// the captured step graph and the force-kernel timer stay as they were.  Nothing outside this file refers to it.
#include "query_pass.hpp"
#include "hist_args.hpp"

using namespace nbh;

namespace nbi {

namespace {

// The hot loop's form when NBODY_HIST_LOOP does not say (profiles/r10_hist_rate.txt): the gated form, which skips the
// windows none of a wave's queries reaches (1.4 - 5.5 x faster where the last edge is a small radius), unless the last edge is +inf —
// then every window with a finite d2 is walked anyway and the first walk is pure cost (4 - 57 %), so the scan it is.
inline int default_loop(bool open_end) { return open_end ? kHistLoopScan : kHistLoopGated; }

// Workgroups per CU a launch of this pass should have before its sources stop being split, in place of query_pass.hpp's kQueryFill = 2:
// measured (profiles/r10_hist_rate.txt), all 65 536 rows of N = 65 536 — 256 workgroups, one per CU — run 2.2 x (4 bins) and 1.26 x (32
// bins) faster over 32 chunks than over the 2 chunks that kQueryFill asks for, and 16 chunks are within 4 % of 32: the loop waits on
// scalar loads, and two workgroups a CU are two waves a SIMD to hide them behind.
constexpr int kHistFill = 16;

// the bytes one rank's sums take in hi_sums, whatever n_bins is: a fixed word, as gather_rank_words wants it
constexpr int kSumsWord = kHistMaxBins * (int)sizeof(unsigned long long);

// a query's edges as the launches take them: HistArgs::edges filled once per call
struct Edges { HistArgs slots; int n_bins; bool open_end; };   // open_end: the last edge is +inf

// NBODY_ERR_ARG for what include/nbody.h refuses: a count outside 1 .. NBODY_HIST_MAX_BINS, a NaN edge, a descending pair
template <typename T>
int check_edges(const T* edges2, int n_bins, Edges& out) {
  if (!edges2 || n_bins < 1 || n_bins > kHistMaxBins) return NBODY_ERR_ARG;
  for (int b = 0; b <= n_bins; ++b) {
    if (edges2[b] != edges2[b]) return NBODY_ERR_ARG;
    if (b > 0 && edges2[b] < edges2[b - 1]) return NBODY_ERR_ARG;
  }
  hist_set_edges<T>(out.slots, edges2, n_bins);
  out.n_bins = n_bins;
  out.open_end = edges2[n_bins] == (T)__builtin_huge_valf();
  return NBODY_OK;
}

int loop_form(const Edges& e) {
  const long long asked = env_ll("NBODY_HIST_LOOP", 0);   // 1: the scan, 2: the gated form (same results), else the default
  return asked == kHistLoopScan || asked == kHistLoopGated ? (int)asked : default_loop(e.open_end);
}

// r.cnt queries on local L — points [r.first, r.first + r.cnt) of the call (already uploaded), or with points == false rows
// [r.first, r.first + r.cnt) of L's slice — with the counts left in hi_count ([r.cnt][n_bins]); L's device is current
int launch_hist(Local& L, bool points, bool skip, const Range& r, const Edges& e) {
  const size_t wb = word_bytes(), nb = (size_t)e.n_bins;
  NBC(L.hi_count.ensure((size_t)r.cnt * nb * sizeof(int)));
  const int n_blocks = source_blocks();
  const int loop = loop_form(e);
  const SplitPlan plan = chunk_split("NBODY_HIST_SPLIT", "NBODY_HIST_SCRATCH_MB", r.cnt, n_blocks, hist_scratch_bytes(1, 1, nb), kHistFill);
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(hist_scratch_bytes((size_t)plan.batch, (size_t)plan.chunks, nb)));
  return for_batches(r.cnt, plan, [&](int b0, int m) {
    HistArgs a = e.slots;
    fill_sources(a, L, plan, n_blocks, m, points ? 0 : L.first + r.first + b0);
    a.points = points ? L.q_points.as<char>() + (size_t)b0 * wb : nullptr;
    a.skip = points && skip ? L.q_skip.as<int>() + b0 : nullptr;
    a.counts = L.hi_count.as<int>() + (size_t)b0 * nb;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<int>() : nullptr;
    a.n_bins = e.n_bins;
    HIPC((hipError_t)nbl::launch_hist_kernel(g.fp64, loop, L.compute, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_hist_combine_kernel(L.compute, a));
    return NBODY_OK;
  });
}

// the queries of a call, rows (points == null) or points, over the locals and their counts into the caller's array
template <typename RangeOf>
int query_impl(RangeOf&& range_of, const void* points, const int* skip, const Edges& e, int* counts) {
  NBC(reconfigure());
  NBC(complete_positions());
  return run_on_locals(range_of,
                       [&](Local& L, const Range& r) {
                         HIPC(hipSetDevice(L.device));
                         if (points) NBC(upload_queries(L, points, skip, r.first, r.cnt));
                         return launch_hist(L, points != nullptr, skip != nullptr, r, e);
                       },
                       [&](Local& L, const Range& r) { return copy_out(counts, r.out, L.hi_count, r.cnt, (size_t)e.n_bins * sizeof(int)); });
}

template <typename T>
int rows_impl(int first_row, int n_rows, const T* edges2, int n_bins, int* counts) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!counts) return NBODY_ERR_ARG;
  Edges e;
  memset(&e, 0, sizeof(e));
  NBC(check_edges(edges2, n_bins, e));
  RowWindow w;   // rows as in nbody_forces_rows
  NBC(w.open(first_row, n_rows));
  return query_impl([&](int l) { return rows_of(w, l); }, nullptr, nullptr, e, counts);
}

template <typename T>
int points_impl(const T* points, int m, const int* skip, const T* edges2, int n_bins, int* counts) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!points || m < 1 || !counts) return NBODY_ERR_ARG;
  Edges e;
  memset(&e, 0, sizeof(e));
  NBC(check_edges(edges2, n_bins, e));
  NBC(check_skip(skip, m));
  return query_impl([&](int l) { return points_of(m, l); }, points, skip, e, counts);
}

// The rows of a batch of the pair histogram: as many as NBODY_HIST_SCRATCH_MB (the bound of chunk_split) allows at n_bins * 4 bytes
// each, in whole workgroups, never fewer than one workgroup's
int pair_batch_rows(int n_bins) {
  const char* mb = getenv("NBODY_HIST_SCRATCH_MB");
  const double bound = std::max(0.0, mb && *mb ? atof(mb) : 256.0) * 1048576.0;
  const double fit = bound / (double)((size_t)n_bins * sizeof(int));
  if (fit >= 2147483647.0) return 2147483647 / nbd::kLanes * nbd::kLanes;
  return std::max(nbd::kLanes, (int)fit / nbd::kLanes * nbd::kLanes);
}

template <typename T>
int pair_impl(const T* edges2, int n_bins, long long* pairs) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!pairs) return NBODY_ERR_ARG;
  Edges e;
  memset(&e, 0, sizeof(e));
  NBC(check_edges(edges2, n_bins, e));
  NBC(reconfigure());
  NBC(complete_positions());
  const int batch = pair_batch_rows(n_bins);
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    HIPC(hipSetDevice(L.device));
    NBC(L.hi_sums.ensure((size_t)g.nranks * kSumsWord));
    unsigned long long* sums = (unsigned long long*)(L.hi_sums.as<char>() + (size_t)L.rank * kSumsWord);
    HIPC(hipMemsetAsync(sums, 0, kSumsWord, L.compute));
    for (int r0 = 0; r0 < L.n_local; r0 += batch) {
      const int rows = std::min(batch, L.n_local - r0);
      NBC(launch_hist(L, false, false, {r0, rows, 0}, e));
      HIPC((hipError_t)nbl::launch_hist_reduce_kernel(L.compute, L.hi_count.as<int>(), rows, n_bins, sums));
    }
  }
  std::vector<unsigned long long> all((size_t)g.nranks * kHistMaxBins, 0ull);
  NBC(gather_rank_words(&Local::hi_sums, all.data(), kSumsWord));
  for (int b = 0; b < n_bins; ++b) {
    unsigned long long twice = 0;
    for (int r = 0; r < g.nranks; ++r) twice += all[(size_t)r * kHistMaxBins + (size_t)b];   // rank order
    pairs[b] = (long long)(twice / 2);   // every pair was counted from both of its rows
  }
  return NBODY_OK;
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_radial_counts_rows(int first_row, int n_rows, const float* edges2, int n_bins, int* counts) { NB_ENTER(0);
  return rows_impl<float>(first_row, n_rows, edges2, n_bins, counts);
}
int nbody_radial_counts_rows_d(int first_row, int n_rows, const double* edges2, int n_bins, int* counts) { NB_ENTER(1);
  return rows_impl<double>(first_row, n_rows, edges2, n_bins, counts);
}
int nbody_radial_counts(const float* points, int m, const int* skip, const float* edges2, int n_bins, int* counts) { NB_ENTER(0);
  return points_impl<float>(points, m, skip, edges2, n_bins, counts);
}
int nbody_radial_counts_d(const double* points, int m, const int* skip, const double* edges2, int n_bins, int* counts) { NB_ENTER(1);
  return points_impl<double>(points, m, skip, edges2, n_bins, counts);
}
int nbody_pair_histogram(const float* edges2, int n_bins, long long* pairs) { NB_ENTER(0);
  return pair_impl<float>(edges2, n_bins, pairs);
}
int nbody_pair_histogram_d(const double* edges2, int n_bins, long long* pairs) { NB_ENTER(1);
  return pair_impl<double>(edges2, n_bins, pairs);
}

}  // extern "C"
