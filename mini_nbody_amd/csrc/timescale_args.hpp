// timescale_args.hpp — what timescale.cpp (host) and timescale.hip (device) agree on: the argument block of the pair time-scale pass and
// the launch functions of timescale.hip.  Like neighbors_args.hpp it stays apart from nbody_args.hpp, the force path's hashed kernel source.
//
// The result of a row (include/nbody.h, "pair time scales") is two minima, both exact, so no order has to be defended: an ascending
// scan over the sources from (tau2 = +inf, idx = -1, d2min = +inf) that replaces on strict <.  When the sources are split over grid.y
// chunks of whole nbd::kSrcBlock-source blocks, every workgroup stores its chunk's {tau2, d2min, idx} and timescale_combine takes the
// chunks in ascending order by the same rule: the same values for every number of chunks.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbts {

struct TimescaleArgs {
  const void* src;      // all N position words (16-B or 32-B {x, y, z, w}), ascending
  const void* vsrc;     // all N velocity words in the same layout: {vx, vy, vz, ignored}
  void* tau2;           // [m] min over j of d2 / v2 in the context precision (+inf: no candidate), or null
  int* idx;             // [m] global index of the j that gives it (-1: none), or null
  void* d2min;          // [m] min over j of d2 (+inf: none), or null
  void* scratch;        // null (grid.y = 1), else the chunks' results: scratch_tau2 / scratch_d2 / scratch_idx below, each
                        // [chunks][m] with row p of chunk c at c * m + p, so that a wave's 64 stores of one field are contiguous
  int n_src;            // N
  int m;                // rows of this launch
  int first;            // global index of row 0: row p is source first + p and leaves itself out
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
  int chunks;           // grid.y = ceil(n_blocks / chunk_blocks): no empty chunk
  // the rows form only: what nbd::query_of reads of a points form is constant here
  static constexpr const void* points = nullptr;
  static constexpr const int* skip = nullptr;
};

// scratch of a launch of m rows over `chunks` chunks: 12 (fp32) or 20 (fp64) bytes per (row, chunk)
inline size_t timescale_scratch_bytes(size_t m, size_t chunks, size_t elem) { return m * chunks * (2 * elem + sizeof(int)); }
__host__ __device__ inline void* scratch_tau2(const TimescaleArgs& a) { return a.scratch; }
__host__ __device__ inline void* scratch_d2(const TimescaleArgs& a, size_t elem) {
  return (char*)a.scratch + (size_t)a.chunks * (size_t)a.m * elem;
}
__host__ __device__ inline int* scratch_idx(const TimescaleArgs& a, size_t elem) {
  return (int*)((char*)a.scratch + 2 * (size_t)a.chunks * (size_t)a.m * elem);
}

// what launch_timescale_kernel refuses
inline bool bad_timescale_launch(const TimescaleArgs& a) { return nbd::bad_source_split(a, true) || !a.src || !a.vsrc; }

// what timescale_best leaves per device or rank: its rows' smallest tau2 with the row i that reaches it first and that row's partner j
// (i < 0: none, tau2 = +inf), and its rows' smallest d2min (+inf: none); both converted exactly to fp64
struct BestScale { double tau2, d2min; int i, j; };

}  // namespace nbts

namespace nbl {
// all return a hipError_t as int (0 = launched; nbd::bad_source_split says what is refused).  grid = (ceil(m / nbd::kLanes), a.chunks);
// a.chunks > 1 is followed by launch_timescale_combine_kernel
int launch_timescale_kernel(int fp64, hipStream_t stream, const nbts::TimescaleArgs& a);
// every row of the launch from a.scratch: chunks ascending, strict < for both minima, then tau2, idx and d2min
int launch_timescale_combine_kernel(int fp64, hipStream_t stream, const nbts::TimescaleArgs& a);
// the best of `rows` rows' (tau2[r], idx[r], d2min[r]), row r being global body first + r: smallest tau2, then lowest row, and the
// smallest d2min, in a fixed order
int launch_timescale_best_kernel(int fp64, hipStream_t stream, const void* tau2, const int* idx, const void* d2min, int rows, int first,
                                 nbts::BestScale* out);
}  // namespace nbl
