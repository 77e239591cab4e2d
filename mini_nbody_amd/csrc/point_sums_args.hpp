// point_sums_args.hpp — what point_sums.cpp (host) and point_sums.hip (device) agree on: the four point-sum passes (the field, the
// tidal tensor, the jerk and the snap of the N bodies at m arbitrary points), their one argument block and the launch functions of point_sums.hip.  Like
// energy_args.hpp it stays apart from nbody_args.hpp, the force path's hashed kernel source.
//
// The order of every sum (include/nbody.h, "field at arbitrary points", "tidal tensor at arbitrary points" and "jerk") is fixed by N alone and
// is the potential's.  A pass has `sums` accumulators per point:
//   level 1  sources in blocks of nbd::kSrcBlock consecutive bodies; per block the accumulators from +0 in ascending j in the context
//            precision; j == skip[p] leaves all of them as they are.
//              field (4)  ax = fma(dx, inv3, ax), ay, az likewise, s = s + inv;
//              tidal (7)  w = 3 inv5, q_ab = fma(w d_a, d_b, q_ab) for ab = xx, yy, zz, xy, xz, yz, s3 = s3 + inv3;
//              jerk (6)   the field's ax, ay, az; with w = v_j - u, b = 3 (d . w) inv2, t_a = fma(-b, d_a, w_a): j_a = fma(t_a, inv3, j_a);
//              snap (9)   the jerk's six; with g = a_j - a (the query's own acceleration), alpha = (d . w) inv2,
//                         q = d . g + w . w (one fma chain), beta = fma(alpha, alpha, q inv2), k6 = 6 alpha, k3 = 3 beta,
//                         u_a = fma(-k3, d_a, fma(-k6, t_a, g_a)): s_a = fma(u_a, inv3, s_a);
//            with masses (PointSumsArgs::masses, m = the w of source j's word): field, jerk and snap take w3 = m * inv3 where inv3 stands
//            above, the tidal w = (3 inv5) * m; s = fma(m, inv, s), s3 = fma(m, inv3, s3).  Nothing else differs.
//   level 2  the blocks' sums converted to fp64 and added in ascending block order from zero, then rounded once.
//              field      accel = (T){A}, phi = (T)(0 - S);
//              tidal      T_aa = (T)(Q_aa - S3), T_ab = (T)Q_ab;
//              jerk       accel = (T){A}, jerk = (T){J};
//              snap       accel = (T){A}, jerk = (T){J}, snap = (T){S}.
// Level 2 happens in registers when one workgroup walks every block of its points (grid.y = 1, scratch == null).  When the sources are
// split over grid.y chunks of whole blocks, every workgroup stores its blocks' level-1 sums — per BLOCK, never per chunk, which is
// what keeps the bits independent of the number of chunks — and the combine kernel adds them.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbp {

// A pass, as the host and the launch functions see it; point_sums.hip states its pair arithmetic and its store.
struct PointPass {
  int id;                       // which of the four
  int sums;                     // kSums: level-1 sums of a point and block
  int out_values[2];            // kOut: values of the context precision per point in each output (0: the pass has no such output)
  const char* split_env;        // the host's variables: the forced number of chunks ...
  const char* scratch_mb_env;   // ... and the bound of the scratch (query_pass.hpp, block_split)
  int velocities;               // 1: the pair reads the velocities of both sides too (vsrc, pvel), and the queries may be rows (first)
  int accelerations;            // 1: ... and the accelerations of both sides (asrc, pacc): a third source stream; needs velocities
  int out2_values;              // values per point in the third output, PointSumsArgs::out2 (0: the pass has none)
};
// field: sums {ax, ay, az, s}; out[0] = accel, words {ax, ay, az, 0}, out[1] = phi; either may be null
inline constexpr PointPass kFieldPass = {0, 4, {4, 1}, "NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB"};
// tidal: sums {qxx, qyy, qzz, qxy, qxz, qyz, s3}; out[0] = the tensor, values {xx, yy, zz, xy, xz, yz}, out[1] stays null
inline constexpr PointPass kTidalPass = {1, 7, {6, 0}, "NBODY_TIDAL_SPLIT", "NBODY_TIDAL_SCRATCH_MB"};
// jerk: sums {ax, ay, az, jx, jy, jz}; out[0] = accel, words {ax, ay, az, 0}, out[1] = jerk, words {jx, jy, jz, 0}; either may be null
inline constexpr PointPass kJerkPass = {2, 6, {4, 4}, "NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB", 1};
// snap: sums {ax, ay, az, jx, jy, jz, sx, sy, sz}; out[0] = accel, out[1] = jerk, out2 = snap, words {., ., ., 0} each; any may be null, not all
inline constexpr PointPass kSnapPass = {3, 9, {4, 4}, "NBODY_SNAP_SPLIT", "NBODY_SNAP_SCRATCH_MB", 1, 1, 4};

struct PointSumsArgs {
  const void* src;      // all N source words (16-B or 32-B {x, y, z, w}), ascending
  const void* points;   // [m] words {x, y, z, ignored} of this launch's points
  const int* skip;      // [m] global body index to leave out, or -1; null: nothing is left out (the kernel's SKIP = false form)
  void* out[2];         // [m][out_values[i]] values in the context precision, as the pass lays them out
  void* scratch;        // null (grid.y = 1), else [n_blocks][sums][m] level-1 sums in the context precision: word (b, q, p) at
                        // (b * sums + q) * m + p, so that a wave's 64 stores of one (b, q) are contiguous
  int n_src;            // N
  int m;                // points of this launch
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
  // a pass with velocities only (the others leave these zero):
  const void* vsrc;     // all N velocity words of the sources, ascending, as src
  const void* pvel;     // [m] words {ux, uy, uz, ignored}: the points' velocities
  int first;            // points == null, the rows form: query p is source first + p — its point src[first + p], its velocity
                        // vsrc[first + p] — and leaves itself out (skip and pvel stay null)
  int masses;           // NBODY_OPT_MASSES: 1 = source j weighs the w of its src word, one more rounding per pair (include/nbody.h); 0 =
                        // unit masses, w is not read.  The w of a points word is ignored either way
  // a pass with accelerations only (the others leave these zero; they stand last, so that the members above keep their offsets):
  void* out2;           // [m][out2_values] values: the third output
  const void* asrc;     // all N acceleration words {ax, ay, az, ignored} of the sources, ascending, as src: the caller brings them
  const void* pacc;     // [m] words {ax, ay, az, ignored}: the points' own accelerations (rows: asrc[first + p])
};

// scratch bytes of a launch of m points (per-block sums: independent of the number of chunks)
inline size_t point_sums_scratch_bytes(size_t m, size_t n_blocks, size_t sums, size_t elem) { return m * n_blocks * sums * elem; }

// what launch_point_sums_kernel and launch_point_sums_combine_kernel refuse: no point, chunks that need scratch and have none, no
// output at all (the block has no `chunks`: the kernel launch takes it beside the block, the combine walks all n_blocks)
inline bool no_point_sums_output(const PointSumsArgs& a) { return !a.out[0] && !a.out[1] && !a.out2; }
inline bool bad_point_sums_launch(const PointSumsArgs& a, int chunks) {
  return a.m <= 0 || chunks < 1 || (chunks > 1 && !a.scratch) || no_point_sums_output(a);
}
inline bool bad_point_sums_combine(const PointSumsArgs& a) { return a.m <= 0 || !a.scratch || no_point_sums_output(a); }
// ... and what the launch refuses of the queries: no points where the pass has no rows form, a pass with velocities without the
// sources' or the points' velocities, a skip array or point velocities beside rows, rows outside the sources; of a pass with
// accelerations the same of the accelerations, and of a pass without them a third output or an acceleration array
inline bool bad_point_sums_queries(const PointPass& pass, const PointSumsArgs& a) {
  if (!pass.accelerations && (a.out2 || a.asrc || a.pacc)) return true;
  if (!pass.velocities) return !a.points;
  if (!a.vsrc || (pass.accelerations && !a.asrc)) return true;
  if (a.points) return !a.pvel || (pass.accelerations && !a.pacc);
  return a.skip || a.pvel || a.pacc || a.first < 0 || a.first > a.n_src - a.m;
}

}  // namespace nbp

namespace nbl {
// both return a hipError_t as int (0 = launched) and refuse a launch with no output at all.  arith: NBODY_ARITH_* (fp64 contexts:
// strict or not).  grid = (ceil(m / nbd::kLanes), chunks); chunks > 1 needs a.scratch and is followed by launch_point_sums_combine_kernel
int launch_point_sums_kernel(const nbp::PointPass& pass, int fp64, int arith, hipStream_t stream, int chunks, const nbp::PointSumsArgs& a);
// level 2 of every point of the launch from a.scratch: blocks ascending in fp64, then the pass's store
int launch_point_sums_combine_kernel(const nbp::PointPass& pass, int fp64, hipStream_t stream, const nbp::PointSumsArgs& a);
}  // namespace nbl
