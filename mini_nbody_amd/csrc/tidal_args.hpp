// tidal_args.hpp — what tidal.cpp (host) and tidal.hip (device) agree on: the argument block of the tidal pass and the launch
// functions of tidal.hip.  Like field_args.hpp it stays apart from nbody_args.hpp, the force path's hashed kernel source.
//
// The order of every sum (include/nbody.h, "tidal tensor at arbitrary points") is fixed by N alone and is the potential's:
//   level 1  sources in blocks of nbd::kSrcBlock consecutive bodies; per block seven accumulators from +0 in ascending j in the context
//            precision: w = 3 inv5, q_ab = fma(w d_a, d_b, q_ab) for ab = xx, yy, zz, xy, xz, yz, s3 = s3 + inv3; j == skip[p] leaves
//            all seven as they are;
//   level 2  the blocks' seven sums converted to fp64 and added in ascending block order from zero: T_aa = (T)(Q_aa - S3), T_ab = (T)Q_ab.
// Level 2 happens in registers when one workgroup walks every block of its points (grid.y = 1, scratch == null).  When the sources are
// split over grid.y chunks of whole blocks, every workgroup stores its blocks' level-1 sums — per BLOCK, never per chunk, which is
// what keeps the bits independent of the number of chunks — and tidal_combine adds them.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbt {

constexpr int kSums = 7;   // level-1 sums of a point and block: {qxx, qyy, qzz, qxy, qxz, qyz, s3}
constexpr int kOut = 6;    // values of a point's result: {xx, yy, zz, xy, xz, yz}

struct TidalArgs {
  const void* src;      // all N source words (16-B or 32-B {x, y, z, w}), ascending
  const void* points;   // [m] words {x, y, z, ignored} of this launch's points
  const int* skip;      // [m] global body index to leave out, or -1; null: nothing is left out (the kernel's SKIP = false form)
  void* tensor;         // [m][kOut] values {xx, yy, zz, xy, xz, yz} in the context precision
  void* scratch;        // null (grid.y = 1), else [n_blocks][kSums][m] level-1 sums in the context precision: word (b, q, p) at
                        // (b * kSums + q) * m + p, so that a wave's 64 stores of one (b, q) are contiguous
  int n_src;            // N
  int m;                // points of this launch
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
};

// scratch bytes of a launch of m points (per-block sums: independent of the number of chunks)
inline size_t tidal_scratch_bytes(size_t m, size_t n_blocks, size_t elem) { return m * n_blocks * kSums * elem; }

}  // namespace nbt

namespace nbl {
// both return a hipError_t as int (0 = launched).  arith: NBODY_ARITH_* (fp64 contexts: strict or not).
// grid = (ceil(m / nbd::kLanes), chunks); chunks > 1 needs a.scratch and is followed by launch_tidal_combine_kernel
int launch_tidal_kernel(int fp64, int arith, hipStream_t stream, int chunks, const nbt::TidalArgs& a);
// level 2 of every point of the launch from a.scratch: blocks ascending in fp64, then the six values
int launch_tidal_combine_kernel(int fp64, hipStream_t stream, const nbt::TidalArgs& a);
}  // namespace nbl
