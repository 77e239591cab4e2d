// diag_pass.hpp — what the diagnostic passes (energy, field, tidal tensor, neighbours, k nearest neighbours, friends-of-friends, radial counts, pair time scales, pair binding energies) share, stated once: the two launch constants their hosts and
// kernels agree on and the guard of a launch over split sources; for device code, the pair arithmetic of the potential, the plain
// squared distance of the six distance passes (neighbours, k nearest neighbours, friends-of-friends, radial counts, pair time scales, pair binding energies), the preamble of a
// one-query-per-lane kernel: the lane, the wave's skip window, the chunk's sources; and the two-stream walk of the two passes that read velocities too (pair_walk).
// energy_args.hpp, point_sums_args.hpp, neighbors_args.hpp, knn_args.hpp, fof_args.hpp, hist_args.hpp, timescale_args.hpp and pair_energy_args.hpp include it.  Like them it stays apart from the force path's hashed
// source (nbody_args.hpp, nbody_kernels.hpp, kernels.hip, force_loop_gfx950.inc), of which it reads nbody_args.hpp (kSoftBits, NB_CONST) only.
// The kernels' loops are different computations and stay in their files; the field's, the tidal tensor's and the jerk's are one (point_sums.hip),
// and so are the pair time-scale and the pair binding-energy pass's (pair_walk below).
#pragma once
#include <hip/hip_runtime.h>

namespace nbd {

constexpr int kSrcBlock = 1024;   // sources per block: a level-1 sum of the potential, the field and the tidal tensor, the unit of a split launch's chunks
constexpr int kLanes = 256;       // lanes per workgroup, one row, point or query each

// What a launch over split sources refuses, for any argument block with the geometry members m, first, n_src, n_blocks, chunk_blocks,
// chunks and scratch: no query, chunks that need scratch and have none, chunks that do not cover the blocks, an empty last chunk, and
// (indexed_by_first: query p is source first + p) a window outside the sources.  Every host split rule normalises to "no empty
// chunk" (query_pass.hpp), so none of this is reachable through include/nbody.h: it guards the launch functions themselves.
template <class A>
inline bool bad_source_split(const A& a, bool indexed_by_first) {
  if (a.m <= 0 || a.chunks < 1 || a.chunk_blocks < 1 || (a.chunks > 1 && !a.scratch)) return true;
  if ((long long)a.chunks * a.chunk_blocks < a.n_blocks || (long long)(a.chunks - 1) * a.chunk_blocks >= a.n_blocks) return true;
  return indexed_by_first && (a.first < 0 || a.first > a.n_src - a.m);
}
// What the combine of a split launch refuses, for any argument block with m, scratch and chunks: no query, no scratch to read, no chunk.
template <class A>
inline bool bad_combine(const A& a) { return a.m <= 0 || !a.scratch || a.chunks < 1; }
// What a reduction over `rows` rows' arrays (a *_best or *_reduce launch) refuses: a negative count, no output, and rows without every
// input array (have_inputs); no rows at all need none.
inline bool bad_row_reduce(int rows, const void* out, bool have_inputs) { return rows < 0 || !out || (rows > 0 && !have_inputs); }
// A pass states its further terms beside its argument block (bad_*_launch, bad_*_combine in its *_args.hpp); the launch functions and
// the host sanitizer harness's stand-ins for them (tests/host_stub) call the same predicates.

}  // namespace nbd

#ifdef __HIP__
#include "nbody_args.hpp"

namespace nbd {

constexpr int kRef = 1, kStrict = 2;   // bits of NBODY_ARITH_*: the reference's d2 roundings, the strict 1/sqrt

__device__ __forceinline__ float fma_of(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_of(double a, double b, double c) { return __builtin_fma(a, b, c); }
// the IEEE minimum of b and a d2 (a NaN d2 gives b): one v_min (two pairs in one v_min3, fp32); both operands are results of
// arithmetic, so nothing is re-quieted
__device__ __forceinline__ float min_of(float b, float d2) { return __builtin_fminf(b, d2); }
__device__ __forceinline__ double min_of(double b, double d2) { return __builtin_fmin(b, d2); }
template <typename T>
__device__ __forceinline__ T inf_of() { return (T)__builtin_huge_valf(); }
template <typename T>
__device__ __forceinline__ T nan_of() { return (T)__builtin_nanf(""); }

template <typename T>
__device__ __forceinline__ T soft() { return (T)__builtin_bit_cast(float, nbk::kSoftBits); }   // the force's eps (S/dzsoft.vhd:177)

// THE statement of (|d|^2 + eps)^(-1/2) for the diagnostic passes, from the three differences, with the force's d2 (nbody_kernels.hpp
// pair_f32): 3 v_fma (FMA3) or the reference's five roundings, then 1 v_rsq_f32.  Strict: the IEEE definition the library's strict
// 1/sqrt is proved equal to (nbody_strict_proof).
template <int ARITH>
__device__ __forceinline__ float inv_dist(float dx, float dy, float dz, float eps) {
  float d2;
  if constexpr (ARITH & kRef) {
    const float sxy = dx * dx + dy * dy;             // S/dxy.vhd:113-122 (compiled with -ffp-contract=off)
    const float sz = __builtin_fmaf(dz, dz, eps);    // S/dzsoft.vhd:201-202
    d2 = sxy + sz;                                   // S/dxyz_soft.vhd:149-150
  } else {
    d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, eps)));
  }
  if constexpr (ARITH & kStrict) return (float)(1.0 / __builtin_sqrt((double)d2));
  else return __builtin_amdgcn_rsqf(d2);             // 1 ulp; d2 >= eps is never subnormal
}
// fp64 (one d2 form, as the force's pair_f64): the v_rsq_f64 seed y refined to full precision by one third-order step,
// with e = 1 - d2 y^2:  d2^(-1/2) = y (1 - e)^(-1/2) = y + y e (1/2 + 3/8 e) + O(e^3);  strict: IEEE sqrt and divide.
// A square that overflows gives d2 = +inf and y = +0, where e = fma(-inf, 0, 1) is NaN: the seed itself is the answer then (+0, as
// the strict form and v_rsq_f32 give).  y == 0 for no finite d2 (d2 >= eps) and not for a NaN d2, which stays NaN.
template <int ARITH>
__device__ __forceinline__ double inv_dist(double dx, double dy, double dz, double eps) {
  const double d2 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, __builtin_fma(dz, dz, eps)));
  if constexpr (ARITH & kStrict) {
    return 1.0 / __builtin_sqrt(d2);
  } else {
    const double y = __builtin_amdgcn_rsq(d2);
    const double e = __builtin_fma(-d2, y * y, 1.0);
    const double r = __builtin_fma(y * e, __builtin_fma(e, 0.375, 0.5), y);
    return y == 0.0 ? y : r;
  }
}

// THE statement of the plain squared distance of a pair, the distance passes' d2: 3 sub, 1 mul, 2 fma.  No softening, one form per
// precision whatever NBODY_OPT_ARITH says, every operation IEEE-exact (their files are compiled with contraction off).
template <typename T, typename V4>
__device__ __forceinline__ T plain_d2(const V4 p, const V4 me) {
  const T dx = p.x - me.x, dy = p.y - me.y, dz = p.z - me.z;
  return fma_of(dx, dx, fma_of(dy, dy, dz * dz));
}
// CMP: the excluded body's (j == sk) d2 becomes a quiet NaN, which is below nothing: neither chosen, counted nor listed
template <bool CMP, typename T, typename V4>
__device__ __forceinline__ T plain_d2(const V4 p, const V4 me, int j, int sk) {
  const T d2 = plain_d2<T, V4>(p, me);
  if (CMP) return j == sk ? nan_of<T>() : d2;
  return d2;
}

// One query per lane, kLanes per workgroup: query p of the launch's m.  Lanes beyond m stay in the wave-uniform loops clamped to the
// last query (pc) and store nothing (live).
struct Lane { int p; bool live; int pc; };
__device__ __forceinline__ Lane lane_of(int m) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  const bool live = p < m;
  return {p, live, live ? p : m - 1};
}

// [lo, hi]: the lowest and highest excluded source index (sk; < 0: none) among the wave's 64 lanes, wave-uniform — only the aligned
// 64-source windows that overlap it have to compare j with sk.  [kNoSkipLo, -1], which no window overlaps, when no lane excludes
// anything, and without a look at the lanes in a kernel's SKIP = false form (whose sk is -1).
constexpr int kNoSkipLo = 0x7fffffff;
struct SkipWindow { int sk, lo, hi; };
template <bool SKIP>
__device__ __forceinline__ SkipWindow wave_skip_window(int sk) {
  if constexpr (SKIP) {
    int lo = sk < 0 ? kNoSkipLo : sk, hi = sk;
    for (int off = 32; off > 0; off >>= 1) {
      lo = min(lo, __shfl_xor(lo, off, 64));
      hi = max(hi, __shfl_xor(hi, off, 64));
    }
    return {sk, __builtin_amdgcn_readfirstlane(lo), __builtin_amdgcn_readfirstlane(hi)};
  } else {
    return {-1, kNoSkipLo, -1};
  }
}

// blocks [b0, b1) of chunk blockIdx.y of a launch whose sources are split into chunks of chunk_blocks whole blocks
struct Blocks { int b0, b1; };
__device__ __forceinline__ Blocks chunk_of(int chunk_blocks, int n_blocks) {
  const int b0 = (int)blockIdx.y * chunk_blocks;
  return {b0, min(b0 + chunk_blocks, n_blocks)};
}
// and its sources [s0, s1), for any argument block with n_src, n_blocks and chunk_blocks
struct Sources { int s0, s1; };
template <class A>
__device__ __forceinline__ Sources chunk_sources(const A& a) {
  const auto [b0, b1] = chunk_of(a.chunk_blocks, a.n_blocks);
  return {b0 * kSrcBlock, min(b1 * kSrcBlock, a.n_src)};
}
// the sources (or their labels) for wave-uniform scalar loads: address space 4
template <typename V>
__device__ __forceinline__ const NB_CONST V* scalar_src(const void* p) { return (const NB_CONST V*)(uintptr_t)p; }

// The preamble of a distance query (lane pc), for any argument block with src, points, skip, first, n_src, n_blocks and chunk_blocks:
// the query point — points[pc], or in the rows form (a.points == null) source a.first + pc, which leaves itself out; SKIP: the
// excluded index and the wave's window of them — the sources and the chunk's range of them.
template <typename V4>
struct Query { V4 me; int sk, wlo, whi; const NB_CONST V4* src; int s0, s1; };
template <typename V4, bool SKIP, class A>
__device__ __forceinline__ Query<V4> query_of(const A& a, int pc) {
  const V4 me = a.points ? ((const V4*)a.points)[pc] : ((const V4*)a.src)[a.first + pc];
  const auto [sk, wlo, whi] = wave_skip_window<SKIP>(!SKIP ? -1 : a.points ? a.skip[pc] : a.first + pc);
  const auto [s0, s1] = chunk_sources(a);
  return {me, sk, wlo, whi, scalar_src<V4>(a.src), s0, s1};
}

// THE walk of the two passes that read two bodies' positions and velocities together (pair time scales: timescale.hip; pair binding
// energies: pair_energy.hip), the body of their hot kernels, for any argument block query_of takes that has vsrc, scratch and m besides.
// One row per lane, kLanes rows per workgroup; workgroup (x, y) walks the blocks of chunk y for the rows of x.  Positions and velocities
// of the sources arrive as two streams of wave-uniform scalar loads (address space 4); the lane's own two words are vector loads.  Lanes
// beyond m stay in the wave-uniform loops clamped to the last row and store nothing.  Only the aligned 64-source windows that overlap
// the wave's own rows [wlo, whi] compare j with the row's index (a wave-uniform branch), and so does the tail (N not a multiple of 64).
// A pass states what differs, as a type P with
//   State                                              what a lane carries: the ascending scan's state
//   static State start()                               the state before the first source
//   static void pair<CMP>(p, u, me, mv, j, sk, State&) the statement of record: one pair (p, u: the source's position and velocity word;
//                                                      me, mv: the row's), CMP as plain_d2's
//   static void to_scratch(a, w, State)                a split launch: the chunk's result of row p at w = chunk * m + p
//   static void to_outputs(a, p, State)                an unsplit launch: row p's results
template <typename V4, class P, class A>
__device__ __forceinline__ void pair_walk(const A& a) {
  const auto [p, live, pc] = lane_of(a.m);
  const auto [me, sk, wlo, whi, src, s0, s1] = query_of<V4, true>(a, pc);
  const V4 mv = ((const V4*)a.vsrc)[a.first + pc];
  const NB_CONST V4* vsrc = scalar_src<V4>(a.vsrc);
  typename P::State c = P::start();
  int j = s0;
  for (; j + 64 <= s1; j += 64) {
    if (j + 63 < wlo || j > whi) {
#pragma unroll 4
      for (int k = 0; k < 64; ++k) P::template pair<false>(src[j + k], vsrc[j + k], me, mv, j + k, sk, c);
    } else {
#pragma unroll 4
      for (int k = 0; k < 64; ++k) P::template pair<true>(src[j + k], vsrc[j + k], me, mv, j + k, sk, c);
    }
  }
  for (; j < s1; ++j) P::template pair<true>(src[j], vsrc[j], me, mv, j, sk, c);
  if (!live) return;
  if (a.scratch) P::to_scratch(a, (size_t)blockIdx.y * (size_t)a.m + (size_t)p, c);
  else P::to_outputs(a, p, c);
}

}  // namespace nbd
#endif  // __HIP__
