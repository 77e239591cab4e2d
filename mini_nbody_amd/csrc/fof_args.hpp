// fof_args.hpp — what fof.cpp (host) and fof.hip (device) agree on: the argument block of the friends-of-friends link pass and the launch
// functions of fof.hip.  Like energy_args.hpp, point_sums_args.hpp, neighbors_args.hpp and knn_args.hpp it stays apart from nbody_args.hpp,
// the force path's hashed kernel source.
//
// One link pass (include/nbody.h, "friends-of-friends groups") gives every row i of the launch the lowest FOREIGN label among its
// friends: m_i = min{ L[j] : d2_ij <= b2 and L[j] != L[i] }, kFoNone when there is none.  An integer minimum is exact, so no order has
// to be defended: when the sources are split over grid.y chunks of whole nbd::kSrcBlock-source blocks, every workgroup stores its chunk's
// minimum and fof_combine takes the minimum over the chunks — the same values for every number of chunks.  The union-find that turns the
// m_i into groups runs on the host (fof.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbg {

constexpr int kFoNone = 0x7fffffff;   // INT_MAX: no friend with a foreign label

struct FofArgs {
  const void* src;      // all N source words (16-B or 32-B {x, y, z, w}), ascending
  const int* label;     // [N] L: the label of every body's current group (its lowest body index)
  const int* rows;      // [m] GLOBAL body index of this launch's rows (the active rows), or null: row p is body first + p
  int* out;             // [m] m_p
  int* scratch;         // null (grid.y = 1), else the chunks' minima [chunks][m]: row p of chunk c at c * m + p, so that a wave's 64
                        // stores are contiguous
  double b2;            // the linking length squared: a value of the context precision, held exactly
  int n_src;            // N
  int m;                // rows of this launch
  int first;            // rows == null: global index of row 0
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
  int chunks;           // grid.y = ceil(n_blocks / chunk_blocks): no empty chunk
};

// scratch of a launch of m rows over `chunks` chunks: 4 bytes per (row, chunk)
inline size_t fof_scratch_bytes(size_t m, size_t chunks) { return m * chunks * sizeof(int); }

// what launch_fof_kernel and launch_fof_combine_kernel refuse
inline bool bad_fof_launch(const FofArgs& a) { return nbd::bad_source_split(a, !a.rows) || !a.src || !a.label || !a.out; }
inline bool bad_fof_combine(const FofArgs& a) { return nbd::bad_combine(a) || !a.out; }

}  // namespace nbg

namespace nbl {
// both return a hipError_t as int (0 = launched; nbd::bad_source_split says what is refused).  grid = (ceil(m / nbd::kLanes), a.chunks); a.chunks > 1 is followed by
// launch_fof_combine_kernel
int launch_fof_kernel(int fp64, hipStream_t stream, const nbg::FofArgs& a);
// every row of the launch from a.scratch: the minimum over the chunks into a.out
int launch_fof_combine_kernel(hipStream_t stream, const nbg::FofArgs& a);
}  // namespace nbl
