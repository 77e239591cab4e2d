// knn_args.hpp — what knn.cpp (host) and knn.hip (device) agree on: the argument block of the k-nearest-neighbour pass and the launch
// functions of knn.hip.  Like energy_args.hpp, point_sums_args.hpp and neighbors_args.hpp it stays apart from nbody_args.hpp, the force
// path's hashed kernel source.
//
// The result of a query (include/nbody.h, "k nearest neighbours") is the first k candidates in ascending (d2, j) order: a selection, so
// it is exact and no order of evaluation has to be defended.  It is what an ascending scan over the sources arrives at that starts from
// k entries (+inf, -1), puts a candidate behind every entry with d2 <= its own and drops the last entry.  When the sources are split
// over grid.y chunks of whole nbd::kSrcBlock-source blocks, every workgroup stores its chunk's k entries and knn_combine pushes the chunks'
// entries, chunks ascending and entries ascending, through the same insertion: lower chunks hold lower j, so the tie rule is kept and
// every number of chunks gives the same values.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbq {

constexpr int kKnMax = 32;   // = NBODY_KNN_MAX: the largest list a lane carries in registers

// the list capacities the kernels are instantiated for; a launch takes the smallest one >= k
constexpr int knn_capacity(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }

struct KnnArgs {
  const void* src;      // all N source words (16-B or 32-B {x, y, z, w}), ascending
  const void* points;   // [m] words {x, y, z, ignored} of this launch's queries; null: the rows form, query p is source first + p
  const int* skip;      // points form: [m] global body index to leave out, or -1; null: nothing is left out.  Rows form: unused
  int* idx;             // [m][k] global indices, entry r of query p at p * k + r (-1: no such candidate), or null
  void* d2;             // [m][k] their squared distances in the context precision (+inf: none), or null
  void* scratch;        // null (grid.y = 1), else the chunks' lists: knn_scratch_d2 / knn_scratch_idx below, each [chunks][k][m] with entry r
                        // of query p of chunk c at (c * k + r) * m + p, so that a wave's 64 stores of one entry are contiguous
  int n_src;            // N
  int m;                // queries of this launch
  int k;                // entries per query, 1 .. kKnMax
  int first;            // rows form: global index of query 0
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
  int chunks;           // grid.y = ceil(n_blocks / chunk_blocks): no empty chunk
};

// scratch of a launch of m queries over `chunks` chunks: k * (elem + 4) bytes per (query, chunk)
inline size_t knn_scratch_bytes(size_t m, size_t chunks, size_t k, size_t elem) { return m * chunks * k * (elem + sizeof(int)); }
__host__ __device__ inline void* knn_scratch_d2(const KnnArgs& a) { return a.scratch; }
__host__ __device__ inline int* knn_scratch_idx(const KnnArgs& a, size_t elem) {
  return (int*)((char*)a.scratch + (size_t)a.chunks * (size_t)a.k * (size_t)a.m * elem);
}
// where entry r of query p of chunk c lies in either array
__host__ __device__ inline size_t knn_scratch_at(const KnnArgs& a, int c, int r, int p) {
  return ((size_t)c * (size_t)a.k + (size_t)r) * (size_t)a.m + (size_t)p;
}

// what launch_knn_kernel and launch_knn_combine_kernel refuse: a k outside 1 .. kKnMax, nowhere to leave the lists
inline bool bad_k(int k) { return k < 1 || k > kKnMax; }
inline bool bad_knn_launch(const KnnArgs& a) { return nbd::bad_source_split(a, !a.points) || bad_k(a.k) || (!a.scratch && !a.idx && !a.d2); }
inline bool bad_knn_combine(const KnnArgs& a) { return nbd::bad_combine(a) || bad_k(a.k) || (!a.idx && !a.d2); }

}  // namespace nbq

namespace nbl {
// both return a hipError_t as int (0 = launched; nbd::bad_source_split says what is refused).  grid = (ceil(m / nbd::kLanes), a.chunks); a.chunks > 1 is followed
// by launch_knn_combine_kernel.  The list capacity is knn_capacity(a.k)
int launch_knn_kernel(int fp64, hipStream_t stream, const nbq::KnnArgs& a);
// every query of the launch from a.scratch: chunks ascending, their entries ascending, the same insertion; then idx and d2
int launch_knn_combine_kernel(int fp64, hipStream_t stream, const nbq::KnnArgs& a);
}  // namespace nbl
