// query_pass.hpp — the host side that the diagnostic passes share (energy.cpp, point_sums.cpp, neighbors.cpp, knn.cpp, fof.cpp, hist.cpp, timescale.cpp, pair_energy.cpp, and hermite.cpp for its gathers; host C++ only): a call brings
// rows or points, every local takes a contiguous range of them, launches on its compute stream — in batches over a split of the
// sources when the pass asks for one — and the results are copied back once the stream has drained.  A pass says what differs: which
// range a local gets, what to launch, which outputs go where, and which of the two split rules (a SplitPlan) it follows: chunk_split,
// for the five distance passes whose scratch is per chunk, or block_split, for the field, tidal and jerk passes, whose scratch is per block.
// The points, skip indices and split scratch of a call live in one set of buffers per Local (q_points, q_skip, q_scratch; q_out, the
// outputs of the field, tidal and jerk passes, and q_vel, the jerk's point velocities, likewise), whichever pass runs: every call drains the streams it used before it returns, so no two calls ever use them at once.
#pragma once
#include "nbody_internal.hpp"
#include "diag_pass.hpp"

namespace nbi {

// Workgroups a launch should have before its sources stop being split, in units of the CU count (see choose_chunks): the starting
// value, not measured yet for the field, neighbour, knn and fof passes (tools/field_rate.py and tools/neighbors_rate.py time the
// passes with and without the split).  Measured for the radial-count pass, where 2 is too few: 256 workgroups of 65 536 rows ran up
// to 2.2 x faster over 16 - 32 chunks than over the 2 this asks for (profiles/r10_hist_rate.txt), so hist.cpp passes its own
// kHistFill = 16 to chunk_split, and timescale.cpp its kTimescaleFill = 16 for the same reason (profiles/r09_timescale.txt).  The same launch shape makes the same question worth asking of the siblings.
constexpr int kQueryFill = 2;

inline long long env_ll(const char* name, long long dflt) {
  const char* e = getenv(name);
  return e && *e ? atoll(e) : dflt;
}

inline size_t elem_bytes() { return g.fp64 ? sizeof(double) : sizeof(float); }
inline int source_blocks() { return (g.n + nbd::kSrcBlock - 1) / nbd::kSrcBlock; }

// C, the number of source chunks (grid.y) of a launch of `queries` queries over n_blocks blocks.  forced >= 1 (the pass's *_SPLIT
// variable): min(forced, n_blocks).  Auto: 1 when the queries alone give kQueryFill workgroups per CU, else the smallest number of
// chunks that does.  fill: the pass's own number in place of kQueryFill, where it has measured one (hist.cpp, timescale.cpp).
inline int choose_chunks(long long forced, int queries, int n_blocks, int fill = kQueryFill) {
  if (forced >= 1) return (int)std::min<long long>(forced, n_blocks);
  const long long groups = ((long long)queries + nbd::kLanes - 1) / nbd::kLanes;
  const long long want = (long long)fill * std::max(1, g.cu_count);
  if (groups >= want) return 1;
  return (int)std::min<long long>((want + groups - 1) / groups, n_blocks);
}

// How a local's launch is cut: grid.y = chunks chunks of chunk_blocks whole blocks (no empty chunk), `batch` queries per launch.
// Two rules make one, chunk_split and block_split below; both fall back to no_split.
struct SplitPlan { int chunks, chunk_blocks, batch; };
inline SplitPlan no_split(int cnt, int n_blocks) { return {1, n_blocks, cnt}; }

// The split of the neighbour, k-nearest-neighbour, friends-of-friends, radial-count and pair time-scale passes, whose scratch is per CHUNK (bytes_per_query_chunk of
// it for every query and chunk): the chunks are chosen from the local's cnt queries — split_env forces their number — and normalised
// first; the queries whose chunk results fit the bound of scratch_mb_env (MB, fractions allowed; 256 when unset) then go together, in
// whole workgroups.
inline SplitPlan chunk_split(const char* split_env, const char* scratch_mb_env, int cnt, int n_blocks, size_t bytes_per_query_chunk,
                             int fill = kQueryFill) {
  const long long forced = env_ll(split_env, 0);
  const char* mb = getenv(scratch_mb_env);
  const double bound = std::max(0.0, mb && *mb ? atof(mb) : 256.0) * 1048576.0;
  const int asked = choose_chunks(forced, cnt, n_blocks, fill);
  if (asked <= 1) return no_split(cnt, n_blocks);
  const int chunk_blocks = (n_blocks + asked - 1) / asked;
  const int chunks = (n_blocks + chunk_blocks - 1) / chunk_blocks;   // no empty chunk
  const double fit = bound / (double)((size_t)chunks * bytes_per_query_chunk);
  int batch = cnt;
  if (fit < (double)cnt) batch = (int)fit / nbd::kLanes * nbd::kLanes;
  if (batch <= 0) return no_split(cnt, n_blocks);   // not one workgroup's queries fit
  return {chunks, chunk_blocks, batch};
}

// The split of the field, tidal and jerk passes, whose scratch is per BLOCK (values level-1 sums of `es` bytes for every point and block:
// point_sums_args.hpp), so its size per point does not depend on the number of chunks: the points whose per-block sums fit
// the bound of scratch_mb_env go together, in whole workgroups, and the chunks are chosen anew for such a batch — split_env forces their
// number.  It reads its MB bound as an integer (env_ll; 256 when unset) where chunk_split takes fractions (atof).
inline SplitPlan block_split(const char* split_env, const char* scratch_mb_env, int cnt, int n_blocks, int values, size_t es) {
  const long long forced = env_ll(split_env, 0);
  const long long bound = std::max<long long>(0, env_ll(scratch_mb_env, 256)) << 20;
  const long long fit = bound / (long long)((size_t)n_blocks * (size_t)values * es) / nbd::kLanes * nbd::kLanes;
  int batch = cnt;
  if (choose_chunks(forced, cnt, n_blocks) > 1 && fit < cnt) batch = (int)fit;   // (fit < 256: batch = 0, no split)
  const int chunks = batch > 0 ? choose_chunks(forced, batch, n_blocks) : 1;
  if (chunks <= 1) return no_split(cnt, n_blocks);
  const int chunk_blocks = (n_blocks + chunks - 1) / chunks;
  return {(n_blocks + chunk_blocks - 1) / chunk_blocks, chunk_blocks, batch};   // no empty chunk
}

// the sources and the geometry members of a distance pass's argument block (diag_pass.hpp's bad_source_split names them) for a launch
// of m queries on local L under plan; first: the global index of query 0 where the queries are rows
template <class A>
void fill_sources(A& a, const Local& L, const SplitPlan& plan, int n_blocks, int m, int first) {
  a.src = L.pos[L.cur];
  a.n_src = g.n;
  a.m = m;
  a.first = first;
  a.n_blocks = n_blocks;
  a.chunk_blocks = plan.chunk_blocks;
  a.chunks = plan.chunks;
}

// launch(b0, m) for the batches [b0, b0 + m) of a local's cnt queries
template <typename Launch>
int for_batches(int cnt, const SplitPlan& plan, Launch&& launch) {
  for (int b0 = 0; b0 < cnt; b0 += plan.batch) NBC(launch(b0, std::min(plan.batch, cnt - b0)));
  return NBODY_OK;
}

// null (nothing is left out) or m indices with -1 <= skip[p] < N
inline int check_skip(const int* skip, int m) {
  if (skip)
    for (int p = 0; p < m; ++p)
      if (skip[p] < -1 || skip[p] >= g.n) return NBODY_ERR_ARG;
  return NBODY_OK;
}

// A local's share of a call: cnt rows of its slice or points of the call from `first`, whose results go to element `out` of the
// caller's arrays (cnt <= 0: the local has no part in the call)
struct Range { int first, cnt, out; };
// m points in contiguous ranges over the locals (one local in an nbody_init_rank context: all of this rank's points)
inline Range points_of(int m, int l) {
  const int p0 = (int)((long long)m * l / g.nlocal), p1 = (int)((long long)m * (l + 1) / g.nlocal);
  return {p0, p1 - p0, p0};
}
// the rows of a window (as nbody_forces_rows takes it) that lie in local l's slice
inline Range rows_of(const RowWindow& w, int l) {
  const Local& L = g.loc[l];
  int r0, cnt;
  if (!w.rows_of(L, &r0, &cnt)) return {0, 0, 0};
  return {r0, cnt, L.first + r0 - w.g0};
}

// points [p0, p0 + cnt) of the call and their skip indices (or null) into L's q_points / q_skip (L's device is current)
// velocities: the points' velocity words (a pass that reads them: the jerk, the snap), into L's q_vel likewise; accelerations: the
// points' acceleration words (the snap), into L's q_acc
inline int upload_queries(Local& L, const void* points, const int* skip, int p0, int cnt, const void* velocities = nullptr,
                          const void* accelerations = nullptr) {
  const size_t wb = word_bytes();
  NBC(L.q_points.ensure((size_t)cnt * wb));
  HIPC(hipMemcpy(L.q_points, (const char*)points + (size_t)p0 * wb, (size_t)cnt * wb, hipMemcpyHostToDevice));
  if (velocities) {
    NBC(L.q_vel.ensure((size_t)cnt * wb));
    HIPC(hipMemcpy(L.q_vel, (const char*)velocities + (size_t)p0 * wb, (size_t)cnt * wb, hipMemcpyHostToDevice));
  }
  if (accelerations) {
    NBC(L.q_acc.ensure((size_t)cnt * wb));
    HIPC(hipMemcpy(L.q_acc, (const char*)accelerations + (size_t)p0 * wb, (size_t)cnt * wb, hipMemcpyHostToDevice));
  }
  if (skip) {
    NBC(L.q_skip.ensure((size_t)cnt * sizeof(int)));
    HIPC(hipMemcpy(L.q_skip, skip + p0, (size_t)cnt * sizeof(int), hipMemcpyHostToDevice));
  }
  return NBODY_OK;
}

// cnt elements of `elem` bytes from the start of dev into element `at` of the caller's array (null: not asked for)
inline int copy_out(void* host, int at, const DevMem& dev, int cnt, size_t elem) {
  if (host) HIPC(hipMemcpy((char*)host + (size_t)at * elem, dev, (size_t)cnt * elem, hipMemcpyDeviceToHost));
  return NBODY_OK;
}

// The two phases of a call, range_of(l) being local l's part in it: launch(L, range) on every local that has one, then per local its
// stream drained and copy_back(L, range): blocking copies into the caller's pageable memory, as the other entry points do
template <typename RangeOf, typename Launch, typename CopyBack>
int run_on_locals(RangeOf&& range_of, Launch&& launch, CopyBack&& copy_back) {
  for (int l = 0; l < g.nlocal; ++l) {
    const Range r = range_of(l);
    if (r.cnt > 0) NBC(launch(g.loc[l], r));
  }
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    const Range r = range_of(l);
    if (r.cnt <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC(hipStreamSynchronize(L.compute));
    NBC(copy_back(L, r));
  }
  return NBODY_OK;
}

// All N words of an array every local holds its own rows of (own_of(L): n_local words in L's device memory) where the kernels of
// every local can read them.  One device: the rows themselves, no copy.  Several devices in one process: every local's L.*all, filled
// by device-to-device copies of the locals' rows (hipMemcpyPeerAsync, as the positions travel in enqueue_gather) on its compute
// stream, which the launch follows.  Several processes: the collective gather of a sharded array into full_scratch with the transport
// in use (gather_sharded_multiprocess) — and, keep: a device copy from there into L.*all, for an array that has to outlive the next
// such gather.  The streams are drained first: a step may still be writing the rows.
template <typename OwnOf>
inline int gather_row_words(OwnOf&& own_of, DevMem Local::*all, bool keep) {
  if (g.nranks == 1) return NBODY_OK;
  NBC(sync_all());
  const size_t wb = word_bytes();
  if (g.multiprocess) {
    Local& L = g.loc[0];
    NBC(gather_sharded_multiprocess(L, own_of(L)));
    if (!keep) return NBODY_OK;
    NBC((L.*all).ensure((size_t)g.n * wb));
    HIPC(hipMemcpyAsync(L.*all, L.full_scratch, (size_t)g.n * wb, hipMemcpyDeviceToDevice, L.compute));
    HIPC(hipStreamSynchronize(L.compute));   // full_scratch is free for the next gather
    return NBODY_OK;
  }
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    HIPC(hipSetDevice(L.device));
    NBC((L.*all).ensure((size_t)g.n * wb));
    for (int o = 0; o < g.nlocal; ++o) {
      const Local& O = g.loc[o];
      if (O.n_local > 0)
        HIPC(hipMemcpyPeerAsync(word_ptr(L.*all, O.first), L.device, own_of(O), O.device, (size_t)O.n_local * wb, L.compute));
    }
  }
  return NBODY_OK;
}

// All N velocity words (the pair time-scale, the pair binding-energy, the jerk and the snap pass): vel itself, every local's ts_vel,
// or full_scratch
inline int gather_velocities() {
  return gather_row_words([](const Local& L) -> const void* { return L.vel; }, &Local::ts_vel, false);
}
inline const void* velocities_of(const Local& L) {
  if (g.nranks == 1) return L.vel;
  return g.multiprocess ? L.full_scratch.as<void>() : L.ts_vel.as<void>();
}

// All N acceleration words (the snap pass) from the own rows' words in L.*own: L.*own itself, or every local's sn_acc_all — in an
// nbody_init_rank job too, where the velocities go through full_scratch next.  Several devices in one process: the copies read every
// owner's buffer on the READERS' streams, so the streams are drained again before anyone may write it (hermite.cpp says the same
// of the velocities).
inline int gather_accelerations(DevMem Local::*own) {
  NBC(gather_row_words([own](const Local& L) -> const void* { return L.*own; }, &Local::sn_acc_all, true));
  if (g.nranks > 1 && !g.multiprocess) NBC(sync_all());
  return NBODY_OK;
}
inline const void* accelerations_of(const Local& L, DevMem Local::*own) {
  return g.nranks == 1 ? (L.*own).as<void>() : L.sn_acc_all.as<void>();
}

// Word `rank` (bytes_per_rank, written on the compute stream) of every rank's L.*buf into host_words[0 .. P): processes exchange the
// words through the transport they use for positions (allgather_rank_words), never a reduction; one process reads each local's own
// word.  The caller folds them in rank order.
inline int gather_rank_words(DevMem Local::*buf, void* host_words, int bytes_per_rank) {
  if (g.multiprocess && g.nranks > 1) return allgather_rank_words(g.loc[0], g.loc[0].*buf, host_words, bytes_per_rank);
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    const size_t off = (size_t)L.rank * (size_t)bytes_per_rank;
    HIPC(hipSetDevice(L.device));
    HIPC(hipStreamSynchronize(L.compute));
    HIPC(hipMemcpy((char*)host_words + off, (L.*buf).as<char>() + off, (size_t)bytes_per_rank, hipMemcpyDeviceToHost));
  }
  return NBODY_OK;
}

// ---- point_sums.cpp ----
// the jerk rows pass over L's own rows into device buffers the caller names (n_local words each), no copy back: see there
int jerk_own_rows_on_device(Local& L, void* accel, void* jerk);
// the jerk points pass over m queries already in L's q_points, q_vel and q_skip, into device buffers likewise (m words each): see there
int jerk_points_on_device(Local& L, int m, void* accel, void* jerk);
// the snap rows pass over L's own rows against the N source accelerations in acc_all (L's device memory), into device buffers
// likewise (n_local words each, any may be null, not all): see there
int snap_own_rows_on_device(Local& L, const void* acc_all, void* accel, void* jerk, void* snap);
// the snap points pass over m queries already in L's q_points, q_vel, q_acc and q_skip against the N source accelerations in acc_all,
// into device buffers likewise (m words each, any may be null, not all): see there
int snap_points_on_device(Local& L, int m, const void* acc_all, void* accel, void* jerk, void* snap);
// what a snap call opens with: the jerk rows pass on every local's own rows into sn_acc and the N accelerations to every device: see there
int snap_open_accelerations();

}  // namespace nbi
