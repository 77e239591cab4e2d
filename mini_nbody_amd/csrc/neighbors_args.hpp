// neighbors_args.hpp — what neighbors.cpp (host) and neighbors.hip (device) agree on: the argument block of the neighbour pass and the
// launch functions of neighbors.hip.  Like energy_args.hpp and point_sums_args.hpp it stays apart from nbody_args.hpp, the force path's
// hashed kernel source.
//
// The result of a query (include/nbody.h, "nearest neighbour, radius count, closest pair") is a minimum and an integer count, both exact,
// so no order has to be defended: an ascending scan over the sources from (d2 = +inf, idx = -1, count = 0) that replaces on strict <.
// When the sources are split over grid.y chunks of whole nbd::kSrcBlock-source blocks, every workgroup stores its chunk's {d2, idx, count}
// and neighbors_combine takes the chunks in ascending order by the same rule (strict <, counts added): the same values for every
// number of chunks.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbn {

// the hot loop's form (same results): SCAN carries (best, index) through every pair; WINDOW keeps only the minimum per aligned
// 64-source window and walks a window again when a lane of the wave improved in it
enum { kNbLoopScan = 1, kNbLoopWindow = 2 };

struct NeighborsArgs {
  const void* src;      // all N source words (16-B or 32-B {x, y, z, w}), ascending
  const void* points;   // [m] words {x, y, z, ignored} of this launch's queries; null: the rows form, query p is source first + p
  const int* skip;      // points form: [m] global body index to leave out, or -1; null: nothing is left out.  Rows form: unused
  int* idx;             // [m] global index of the nearest body (-1: none), or null
  void* d2;             // [m] its squared distance in the context precision (+inf: none), or null
  int* count;           // [m] bodies with d2_j <= r2, or null (the kernel's COUNT = false form)
  void* scratch;        // null (grid.y = 1), else the chunks' results: scratch_d2 / scratch_idx / scratch_count below, each
                        // [chunks][m] with query p of chunk c at c * m + p, so that a wave's 64 stores of one field are contiguous
  double r2;            // the radius squared: a value of the context precision, held exactly
  int n_src;            // N
  int m;                // queries of this launch
  int first;            // rows form: global index of query 0
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
  int chunks;           // grid.y = ceil(n_blocks / chunk_blocks): no empty chunk
};

// scratch of a launch of m queries over `chunks` chunks: 12 (fp32) or 16 (fp64) bytes per (query, chunk)
inline size_t neighbors_scratch_bytes(size_t m, size_t chunks, size_t elem) { return m * chunks * (elem + 2 * sizeof(int)); }
__host__ __device__ inline void* scratch_d2(const NeighborsArgs& a) { return a.scratch; }
__host__ __device__ inline int* scratch_idx(const NeighborsArgs& a, size_t elem) {
  return (int*)((char*)a.scratch + (size_t)a.chunks * (size_t)a.m * elem);
}
__host__ __device__ inline int* scratch_count(const NeighborsArgs& a, size_t elem) { return scratch_idx(a, elem) + (size_t)a.chunks * (size_t)a.m; }

// what neighbors_best leaves per device or rank: its rows' closest pair (i < 0: none, d2 = +inf); d2 converted exactly to fp64
struct BestPair { double d2; int i, j; };

}  // namespace nbn

namespace nbl {
// all return a hipError_t as int (0 = launched; nbd::bad_source_split says what is refused).  grid = (ceil(m / nbd::kLanes), a.chunks); a.chunks > 1 is followed
// by launch_neighbors_combine_kernel.  loop: kNbLoopScan or kNbLoopWindow
int launch_neighbors_kernel(int fp64, int loop, hipStream_t stream, const nbn::NeighborsArgs& a);
// every query of the launch from a.scratch: chunks ascending, strict <, counts added, then idx, d2 and count
int launch_neighbors_combine_kernel(int fp64, hipStream_t stream, const nbn::NeighborsArgs& a);
// the best of `rows` rows' (d2[r], idx[r]), row r being global body first + r: smallest d2, then lowest row, in a fixed order
int launch_neighbors_best_kernel(int fp64, hipStream_t stream, const void* d2, const int* idx, int rows, int first, nbn::BestPair* out);
}  // namespace nbl
