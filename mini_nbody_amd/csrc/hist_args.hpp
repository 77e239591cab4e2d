// hist_args.hpp — what hist.cpp (host) and hist.hip (device) agree on: the argument block of the radial-count pass and the launch
// functions of hist.hip.  Like energy_args.hpp, point_sums_args.hpp, neighbors_args.hpp, knn_args.hpp and fof_args.hpp it stays apart from
// nbody_args.hpp, the force path's hashed kernel source.
//
// The result of a query (include/nbody.h, "radial counts, pair histogram") is n_bins integers, differences of the cumulative counts
// c_b = #{ j : d2_j < edges2[b] }: exact, so no order of evaluation has to be defended.  When the sources are split over grid.y chunks
// of whole nbd::kSrcBlock-source blocks, every workgroup stores its chunk's n_bins counts and hist_combine adds the chunks' counts per
// (query, bin): the same values for every number of chunks.  The pair histogram adds the rows' counts of a device into n_bins 64-bit
// sums with integer atomics (hist_reduce): integer sums, the same values in every order.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbh {

constexpr int kHistMaxBins = 32;                 // = NBODY_HIST_MAX_BINS: the most counters a lane carries in registers
constexpr int kHistSlots = kHistMaxBins + 1;     // edges of the largest query

// the bin capacities the kernels are instantiated for; a launch takes the smallest one >= n_bins (capacity C: C + 1 edge slots)
constexpr int hist_capacity(int n_bins) { return n_bins <= 4 ? 4 : n_bins <= 8 ? 8 : n_bins <= 16 ? 16 : 32; }

// the hot loop's form (same results): SCAN compares every pair with every edge; GATED first takes the running minimum of an aligned
// 64-source window alone and walks the window with the counters only if a lane of the wave has a d2 below the last edge
enum { kHistLoopScan = 1, kHistLoopGated = 2 };

struct HistArgs {
  const void* src;      // all N source words (16-B or 32-B {x, y, z, w}), ascending
  const void* points;   // [m] words {x, y, z, ignored} of this launch's queries; null: the rows form, query p is source first + p
  const int* skip;      // points form: [m] global body index to leave out, or -1; null: nothing is left out.  Rows form: unused
  int* counts;          // [m][n_bins] bin b of query p at p * n_bins + b
  int* scratch;         // null (grid.y = 1), else the chunks' counts: [chunks][n_bins][m] with bin b of query p of chunk c at
                        // hist_scratch_at below, so that a wave's 64 stores of one bin are contiguous
  // kHistSlots values of the context precision (a float or a double each, at slot * sizeof(T)), right-aligned: the query's
  // n_bins + 1 squared radii are the LAST n_bins + 1 slots and every slot before them holds -inf, which nothing is below.  A kernel of
  // capacity C reads the last C + 1 slots, each at a constant offset
  alignas(8) unsigned char edges[kHistSlots * sizeof(double)];
  int n_src;            // N
  int m;                // queries of this launch
  int n_bins;           // bins per query, 1 .. kHistMaxBins
  int first;            // rows form: global index of query 0
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
  int chunks;           // grid.y = ceil(n_blocks / chunk_blocks): no empty chunk
};

// scratch of a launch of m queries over `chunks` chunks: n_bins * 4 bytes per (query, chunk)
inline size_t hist_scratch_bytes(size_t m, size_t chunks, size_t n_bins) { return m * chunks * n_bins * sizeof(int); }
// where bin b of query p of chunk c lies in it
__host__ __device__ inline size_t hist_scratch_at(const HistArgs& a, int c, int b, int p) {
  return ((size_t)c * (size_t)a.n_bins + (size_t)b) * (size_t)a.m + (size_t)p;
}

// the edges of a query into a.edges, T being the context precision
template <typename T>
inline void hist_set_edges(HistArgs& a, const T* edges2, int n_bins) {
  T* slot = (T*)a.edges;
  const int lead = kHistSlots - (n_bins + 1);
  for (int s = 0; s < kHistSlots; ++s) slot[s] = s < lead ? -(T)__builtin_huge_valf() : edges2[s - lead];
}

// what the three launch functions refuse: an n_bins outside 1 .. kHistMaxBins, nowhere to leave the counts
inline bool bad_bins(int n_bins) { return n_bins < 1 || n_bins > kHistMaxBins; }
inline bool bad_hist_launch(const HistArgs& a) { return nbd::bad_source_split(a, !a.points) || bad_bins(a.n_bins) || (!a.scratch && !a.counts); }
inline bool bad_hist_combine(const HistArgs& a) { return nbd::bad_combine(a) || bad_bins(a.n_bins) || !a.counts; }
inline bool bad_hist_reduce(const int* counts, int rows, int n_bins, const unsigned long long* sums) {
  return bad_bins(n_bins) || nbd::bad_row_reduce(rows, sums, counts != nullptr);
}

}  // namespace nbh

namespace nbl {
// all return a hipError_t as int (0 = launched; nbd::bad_source_split says what is refused).  grid = (ceil(m / nbd::kLanes), a.chunks);
// a.chunks > 1 is followed by launch_hist_combine_kernel.  The capacity is hist_capacity(a.n_bins); loop: kHistLoopScan or kHistLoopGated
int launch_hist_kernel(int fp64, int loop, hipStream_t stream, const nbh::HistArgs& a);
// every query of the launch from a.scratch: the chunks' counts added per (query, bin), then counts
int launch_hist_combine_kernel(hipStream_t stream, const nbh::HistArgs& a);
// sums[b] += the sum over `rows` rows of counts[r * n_bins + b], b < n_bins; the caller zeroes sums before the first batch
int launch_hist_reduce_kernel(hipStream_t stream, const int* counts, int rows, int n_bins, unsigned long long* sums);
}  // namespace nbl
