// field_args.hpp — what field.cpp (host) and field.hip (device) agree on: the argument block of the field pass and the launch
// functions of field.hip.  Like energy_args.hpp it stays apart from nbody_args.hpp, the force path's hashed kernel source.
//
// The order of every sum (include/nbody.h, "field at arbitrary points") is fixed by N alone and is the potential's:
//   level 1  sources in blocks of nbd::kSrcBlock consecutive bodies; per block four accumulators from +0 in ascending j in the context
//            precision: ax = fma(dx, inv3, ax), ay, az likewise, s = s + inv; j == skip[p] leaves all four as they are;
//   level 2  the blocks' four sums converted to fp64 and added in ascending block order from zero: accel = (T){A}, phi = (T)(0 - S).
// Level 2 happens in registers when one workgroup walks every block of its points (grid.y = 1, scratch == null).  When the sources are
// split over grid.y chunks of whole blocks, every workgroup stores its blocks' level-1 sums — per BLOCK, never per chunk, which is
// what keeps the bits independent of the number of chunks — and field_combine adds them.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbf {

struct FieldArgs {
  const void* src;      // all N source words (16-B or 32-B {x, y, z, w}), ascending
  const void* points;   // [m] words {x, y, z, ignored} of this launch's points
  const int* skip;      // [m] global body index to leave out, or -1; null: nothing is left out (the kernel's SKIP = false form)
  void* accel;          // [m] words {ax, ay, az, 0} in the context precision, or null
  void* phi;            // [m] values in the context precision, or null
  void* scratch;        // null (grid.y = 1), else [n_blocks][4][m] level-1 sums in the context precision: word (b, q, p) at
                        // (b * 4 + q) * m + p, q = {ax, ay, az, s}, so that a wave's 64 stores of one (b, q) are contiguous
  int n_src;            // N
  int m;                // points of this launch
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
};

// scratch bytes of a launch of m points (per-block sums: independent of the number of chunks)
inline size_t field_scratch_bytes(size_t m, size_t n_blocks, size_t elem) { return m * n_blocks * 4 * elem; }

}  // namespace nbf

namespace nbl {
// both return a hipError_t as int (0 = launched).  arith: NBODY_ARITH_* (fp64 contexts: strict or not).
// grid = (ceil(m / nbd::kLanes), chunks); chunks > 1 needs a.scratch and is followed by launch_field_combine_kernel
int launch_field_kernel(int fp64, int arith, hipStream_t stream, int chunks, const nbf::FieldArgs& a);
// level 2 of every point of the launch from a.scratch: blocks ascending in fp64, then accel and phi
int launch_field_combine_kernel(int fp64, hipStream_t stream, const nbf::FieldArgs& a);
}  // namespace nbl
