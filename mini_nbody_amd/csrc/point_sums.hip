// point_sums.hip — the device code of the four point-sum passes: the field (acceleration and potential), the tidal tensor T = grad a =
// -grad grad phi, the jerk da/dt and the snap d2a/dt2 of the N bodies on the device at m arbitrary points or rows (point_sums_args.hpp states the order,
// include/nbody.h the definitions).  One skeleton — a kernel of blocked level-1 sums, its combine, one launcher pair — and a statement per pass of what
// differs: the number of sums, the pair, the store.  Compiles on its own; device.hip puts it into the library's one code object after
// kernels.hip and energy.hip.  Reads nbody_args.hpp (f4, d4, NB_CONST) and nothing else of the force path: d2 and 1/sqrt are
// diag_pass.hpp's inv_dist, the potential's; the field's cube and three fma follow the force's pair_f32 / pair_f64.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "point_sums_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbp;
using namespace nbd;

#define NBP_HIDDEN __attribute__((visibility("hidden")))

namespace {

// ---- the pass statements.  pair: one source into the level-1 sums c of a point; every intermediate comes before the CMP return, which
// ---- keeps the CMP = false body free of branches; CMP: source j == sk leaves c as it is.  store: a point's result from its level-2 sums.

// MASS (NBODY_OPT_MASSES = 1): the one extra rounding of a pair, m = the w of the source's word as it lies in src — x * m in this
// operand order; MASS = false is x itself, so that the unweighted instantiations are what they were
template <bool MASS, typename T>
__device__ __forceinline__ T weighted(T m, T x) { if constexpr (MASS) return x * m; else return x; }

struct FieldSums {
  static constexpr int kSums = kFieldPass.sums;   // {ax, ay, az, s}
  static constexpr bool kVel = kFieldPass.velocities, kAcc = kFieldPass.accelerations;
  // 3 sub, d2, 1/sqrt, 2 mul (the force's cube), 3 fma, 1 add; MASS: 1 mul (w3 = m inv3) more, and the add is an fma
  template <int ARITH, bool CMP, bool MASS, typename T, typename V4>
  static __device__ __forceinline__ void pair(const V4 p, const V4 me, T eps, int j, int sk, T (&c)[kSums]) {
    const T dx = p.x - me.x, dy = p.y - me.y, dz = p.z - me.z;
    const T inv = inv_dist<ARITH>(dx, dy, dz, eps);
    const T inv2 = inv * inv;
    const T inv3 = inv * inv2;
    const T w3 = weighted<MASS>(p.w, inv3);
    const T ax = fma_of(dx, w3, c[0]), ay = fma_of(dy, w3, c[1]), az = fma_of(dz, w3, c[2]), s = MASS ? fma_of(p.w, inv, c[3]) : c[3] + inv;
    if (CMP && j == sk) return;
    c[0] = ax; c[1] = ay; c[2] = az; c[3] = s;
  }
  template <typename T, typename V4>
  static __device__ __forceinline__ void store(const PointSumsArgs& a, int p, const double (&l2)[kSums]) {
    if (a.out[0]) ((V4*)a.out[0])[p] = V4{(T)l2[0], (T)l2[1], (T)l2[2], (T)0};
    if (a.out[1]) ((T*)a.out[1])[p] = (T)(0.0 - l2[3]);
  }
};

struct TidalSums {
  static constexpr int kSums = kTidalPass.sums;   // {qxx, qyy, qzz, qxy, qxz, qyz, s3}
  static constexpr bool kVel = kTidalPass.velocities, kAcc = kTidalPass.accelerations;
  // 3 sub, d2, 1/sqrt, 3 mul (inv2, inv3, inv5), 1 mul (w = 3 inv5), 3 mul (w d), 6 fma, 1 add: 21 VALU + 1 transcendental in the fp32
  // timed form; MASS: 1 mul (w = (3 inv5) m) more, and the add is an fma
  template <int ARITH, bool CMP, bool MASS, typename T, typename V4>
  static __device__ __forceinline__ void pair(const V4 p, const V4 me, T eps, int j, int sk, T (&c)[kSums]) {
    const T dx = p.x - me.x, dy = p.y - me.y, dz = p.z - me.z;
    const T inv = inv_dist<ARITH>(dx, dy, dz, eps);
    const T inv2 = inv * inv;
    const T inv3 = inv * inv2;
    const T inv5 = inv3 * inv2;
    const T w = weighted<MASS>(p.w, (T)3 * inv5);
    const T wx = w * dx, wy = w * dy, wz = w * dz;
    const T xx = fma_of(wx, dx, c[0]), yy = fma_of(wy, dy, c[1]), zz = fma_of(wz, dz, c[2]);
    const T xy = fma_of(wx, dy, c[3]), xz = fma_of(wx, dz, c[4]), yz = fma_of(wy, dz, c[5]);
    const T s3 = MASS ? fma_of(p.w, inv3, c[6]) : c[6] + inv3;
    if (CMP && j == sk) return;
    c[0] = xx; c[1] = yy; c[2] = zz; c[3] = xy; c[4] = xz; c[5] = yz; c[6] = s3;
  }
  // the six values {xx, yy, zz, xy, xz, yz}: the diagonal's subtraction in fp64, rounded once
  template <typename T, typename V4>
  static __device__ __forceinline__ void store(const PointSumsArgs& a, int p, const double (&l2)[kSums]) {
    T* out = (T*)a.out[0] + (size_t)p * kTidalPass.out_values[0];
    out[0] = (T)(l2[0] - l2[6]); out[1] = (T)(l2[1] - l2[6]); out[2] = (T)(l2[2] - l2[6]);
    out[3] = (T)l2[3]; out[4] = (T)l2[4]; out[5] = (T)l2[5];
  }
};

struct JerkSums {
  static constexpr int kSums = kJerkPass.sums;   // {ax, ay, az, jx, jy, jz}
  static constexpr bool kVel = kJerkPass.velocities, kAcc = kJerkPass.accelerations;   // pair takes the two velocities beside the two positions
  // 6 sub, d2, 1/sqrt, 2 mul (the cube), 1 mul + 2 fma (d . w), 2 mul (3 rv, inv2), 3 fma (t), 3 fma (the field's), 3 fma: 25 VALU + 1
  // transcendental in the fp32 timed form; MASS: 1 mul (w3 = m inv3) more.  p, me: positions; u, mv: velocities of the source and of the query
  template <int ARITH, bool CMP, bool MASS, typename T, typename V4>
  static __device__ __forceinline__ void pair(const V4 p, const V4 u, const V4 me, const V4 mv, T eps, int j, int sk, T (&c)[kSums]) {
    const T dx = p.x - me.x, dy = p.y - me.y, dz = p.z - me.z;
    const T wx = u.x - mv.x, wy = u.y - mv.y, wz = u.z - mv.z;
    const T inv = inv_dist<ARITH>(dx, dy, dz, eps);
    const T inv2 = inv * inv;
    const T inv3 = inv * inv2;
    const T rv = fma_of(dx, wx, fma_of(dy, wy, dz * wz));
    const T b = ((T)3 * rv) * inv2;
    const T tx = fma_of(-b, dx, wx), ty = fma_of(-b, dy, wy), tz = fma_of(-b, dz, wz);
    const T w3 = weighted<MASS>(p.w, inv3);
    const T ax = fma_of(dx, w3, c[0]), ay = fma_of(dy, w3, c[1]), az = fma_of(dz, w3, c[2]);
    const T jx = fma_of(tx, w3, c[3]), jy = fma_of(ty, w3, c[4]), jz = fma_of(tz, w3, c[5]);
    if (CMP && j == sk) return;
    c[0] = ax; c[1] = ay; c[2] = az; c[3] = jx; c[4] = jy; c[5] = jz;
  }
  template <typename T, typename V4>
  static __device__ __forceinline__ void store(const PointSumsArgs& a, int p, const double (&l2)[kSums]) {
    if (a.out[0]) ((V4*)a.out[0])[p] = V4{(T)l2[0], (T)l2[1], (T)l2[2], (T)0};
    if (a.out[1]) ((V4*)a.out[1])[p] = V4{(T)l2[3], (T)l2[4], (T)l2[5], (T)0};
  }
};

struct SnapSums {
  static constexpr int kSums = kSnapPass.sums;   // {ax, ay, az, jx, jy, jz, sx, sy, sz}
  static constexpr bool kVel = kSnapPass.velocities, kAcc = kSnapPass.accelerations;   // pair takes the two accelerations beside positions and velocities
  // JerkSums::pair to the letter (d, w, inv, inv2, inv3, rv, b, t, the six fma: accel and jerk are the jerk pass's bits), then 3 sub (g),
  // 1 mul (alpha), 1 mul + 5 fma (q), 1 mul + 1 fma (beta), 2 mul (k6, k3), 6 fma (u), 3 fma: 48 VALU + 1 transcendental in the fp32
  // timed form; MASS: the jerk's one mul.  h, ma: accelerations of the source and of the query
  template <int ARITH, bool CMP, bool MASS, typename T, typename V4>
  static __device__ __forceinline__ void pair(const V4 p, const V4 u, const V4 h, const V4 me, const V4 mv, const V4 ma, T eps, int j, int sk,
                                              T (&c)[kSums]) {
    const T dx = p.x - me.x, dy = p.y - me.y, dz = p.z - me.z;
    const T wx = u.x - mv.x, wy = u.y - mv.y, wz = u.z - mv.z;
    const T inv = inv_dist<ARITH>(dx, dy, dz, eps);
    const T inv2 = inv * inv;
    const T inv3 = inv * inv2;
    const T rv = fma_of(dx, wx, fma_of(dy, wy, dz * wz));
    const T b = ((T)3 * rv) * inv2;
    const T tx = fma_of(-b, dx, wx), ty = fma_of(-b, dy, wy), tz = fma_of(-b, dz, wz);
    const T w3 = weighted<MASS>(p.w, inv3);
    const T ax = fma_of(dx, w3, c[0]), ay = fma_of(dy, w3, c[1]), az = fma_of(dz, w3, c[2]);
    const T jx = fma_of(tx, w3, c[3]), jy = fma_of(ty, w3, c[4]), jz = fma_of(tz, w3, c[5]);
    const T gx = h.x - ma.x, gy = h.y - ma.y, gz = h.z - ma.z;
    const T alpha = rv * inv2;
    const T q = fma_of(dx, gx, fma_of(dy, gy, fma_of(dz, gz, fma_of(wx, wx, fma_of(wy, wy, wz * wz)))));
    const T beta = fma_of(alpha, alpha, q * inv2);
    const T k6 = (T)6 * alpha, k3 = (T)3 * beta;
    const T ux = fma_of(-k3, dx, fma_of(-k6, tx, gx)), uy = fma_of(-k3, dy, fma_of(-k6, ty, gy)), uz = fma_of(-k3, dz, fma_of(-k6, tz, gz));
    const T sx = fma_of(ux, w3, c[6]), sy = fma_of(uy, w3, c[7]), sz = fma_of(uz, w3, c[8]);
    if (CMP && j == sk) return;
    c[0] = ax; c[1] = ay; c[2] = az; c[3] = jx; c[4] = jy; c[5] = jz; c[6] = sx; c[7] = sy; c[8] = sz;
  }
  template <typename T, typename V4>
  static __device__ __forceinline__ void store(const PointSumsArgs& a, int p, const double (&l2)[kSums]) {
    if (a.out[0]) ((V4*)a.out[0])[p] = V4{(T)l2[0], (T)l2[1], (T)l2[2], (T)0};
    if (a.out[1]) ((V4*)a.out[1])[p] = V4{(T)l2[3], (T)l2[4], (T)l2[5], (T)0};
    if (a.out2) ((V4*)a.out2)[p] = V4{(T)l2[6], (T)l2[7], (T)l2[8], (T)0};
  }
};

// ---- the skeleton ----

// The query of lane pc: its point, (a pass with velocities) its velocity, (a pass with accelerations) its acceleration, and the source
// it leaves out (SKIP = false: -1).  A pass with velocities also has the rows form (a.points == null): query pc is source a.first + pc,
// read from src and vsrc (and asrc), and leaves itself out.
template <typename V4>
struct QueryWords { V4 me, mv; int own; };
template <class P, typename V4>
__device__ __forceinline__ V4 query_acc(const PointSumsArgs& a, int pc) {
  if constexpr (P::kAcc) return a.points ? ((const V4*)a.pacc)[pc] : ((const V4*)a.asrc)[a.first + pc];
  else return V4{};
}
template <class P, typename V4, bool SKIP>
__device__ __forceinline__ QueryWords<V4> query_words(const PointSumsArgs& a, int pc) {
  if constexpr (P::kVel) {
    if (!a.points) return {((const V4*)a.src)[a.first + pc], ((const V4*)a.vsrc)[a.first + pc], SKIP ? a.first + pc : -1};
    return {((const V4*)a.points)[pc], ((const V4*)a.pvel)[pc], SKIP ? a.skip[pc] : -1};
  } else {
    return {((const V4*)a.points)[pc], V4{}, SKIP ? a.skip[pc] : -1};
  }
}

// source j into the sums c: its position, (a pass with velocities) its velocity and (a pass with accelerations) its acceleration, all
// wave-uniform scalar loads
template <class P, int ARITH, bool CMP, bool MASS, typename T, typename V4>
__device__ __forceinline__ void pair_of(const NB_CONST V4* src, const NB_CONST V4* vsrc, const NB_CONST V4* asrc, int j, const V4 me,
                                        const V4 mv, const V4 ma, T eps, int sk, T (&c)[P::kSums]) {
  if constexpr (P::kAcc) P::template pair<ARITH, CMP, MASS, T, V4>(src[j], vsrc[j], asrc[j], me, mv, ma, eps, j, sk, c);
  else if constexpr (P::kVel) P::template pair<ARITH, CMP, MASS, T, V4>(src[j], vsrc[j], me, mv, eps, j, sk, c);
  else P::template pair<ARITH, CMP, MASS, T, V4>(src[j], me, eps, j, sk, c);
}

// One point per lane, kLanes points per workgroup; workgroup (x, y) walks the blocks of chunk y for the points of x.  Sources
// arrive with wave-uniform scalar loads (address space 4, as energy_kernel) — in a pass with velocities as two streams, positions and
// velocities, as timescale_kernel's, in a pass with accelerations as three.  Lanes beyond m stay in the wave-uniform loops clamped to
// the last point and store nothing.  SKIP: only the aligned 64-source windows that overlap [lowest, highest] skip index of the wave's
// 64 points compare j with skip (a wave-uniform branch); every other window, and every window of the SKIP = false form, is the pass's
// branch-free pair (field: 3 sub, 3 fma, 1 rsq, 2 mul, 3 fma and 1 add).
template <class P, typename T, typename V4, int ARITH, bool SKIP, bool MASS>
__global__ void __launch_bounds__(kLanes) block_sums_kernel(PointSumsArgs a) {
  constexpr int S = P::kSums;
  const auto [p, live, pc] = lane_of(a.m);
  const auto [me, mv, own] = query_words<P, V4, SKIP>(a, pc);
  const V4 ma = query_acc<P, V4>(a, pc);
  const auto [sk, wlo, whi] = wave_skip_window<SKIP>(own);
  const T eps = soft<T>();
  const NB_CONST V4* src = scalar_src<V4>(a.src);
  const NB_CONST V4* vsrc = scalar_src<V4>(P::kVel ? a.vsrc : nullptr);
  const NB_CONST V4* asrc = scalar_src<V4>(P::kAcc ? a.asrc : nullptr);
  T* sc = (T*)a.scratch;
  const auto [blk0, blk1] = chunk_of(a.chunk_blocks, a.n_blocks);
  double l2[S] = {};
  for (int blk = blk0; blk < blk1; ++blk) {
    const int b0 = blk * kSrcBlock;
    const int b1 = min(b0 + kSrcBlock, a.n_src);
    T c[S] = {};
    int j = b0;
    for (; j + 64 <= b1; j += 64) {
      if (!SKIP || j + 63 < wlo || j > whi) {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) pair_of<P, ARITH, false, MASS, T, V4>(src, vsrc, asrc, j + k, me, mv, ma, eps, sk, c);
      } else {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) pair_of<P, ARITH, true, MASS, T, V4>(src, vsrc, asrc, j + k, me, mv, ma, eps, sk, c);
      }
    }
    for (; j < b1; ++j) pair_of<P, ARITH, SKIP, MASS, T, V4>(src, vsrc, asrc, j, me, mv, ma, eps, sk, c);   // the last block's tail (N not a multiple of 64)
    if (sc) {
      if (live) {
        const size_t w = (size_t)blk * S * (size_t)a.m + (size_t)p;
#pragma unroll
        for (int q = 0; q < S; ++q) sc[w + (size_t)q * (size_t)a.m] = c[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < S; ++q) l2[q] += (double)c[q];
    }
  }
  if (!sc && live) P::template store<T, V4>(a, p, l2);
}

// level 2 from the stored per-block sums: blocks ascending, fp64, one point per lane (a wave reads 64 consecutive values per word)
template <class P, typename T, typename V4>
__global__ void __launch_bounds__(kLanes) block_sums_combine(PointSumsArgs a) {
  constexpr int S = P::kSums;
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.m) return;
  const T* sc = (const T*)a.scratch;
  const size_t m = (size_t)a.m;
  double l2[S] = {};
  for (int blk = 0; blk < a.n_blocks; ++blk) {
    const size_t w = (size_t)blk * S * m + (size_t)p;
#pragma unroll
    for (int q = 0; q < S; ++q) l2[q] += (double)sc[w + (size_t)q * m];
  }
  P::template store<T, V4>(a, p, l2);
}

template <class P, typename T, typename V4, int ARITH, bool MASS>
void launch_sums_one(hipStream_t st, int chunks, const PointSumsArgs& a) {
  const dim3 grid((a.m + kLanes - 1) / kLanes, chunks);
  if (a.skip || !a.points) hipLaunchKernelGGL((block_sums_kernel<P, T, V4, ARITH, true, MASS>), grid, dim3(kLanes), 0, st, a);   // (rows leave themselves out)
  else hipLaunchKernelGGL((block_sums_kernel<P, T, V4, ARITH, false, MASS>), grid, dim3(kLanes), 0, st, a);
}

template <class P, typename T, typename V4, int ARITH>
void launch_sums_one(hipStream_t st, int chunks, const PointSumsArgs& a) {
  if (a.masses) launch_sums_one<P, T, V4, ARITH, true>(st, chunks, a);
  else launch_sums_one<P, T, V4, ARITH, false>(st, chunks, a);
}

template <class P>
int launch_sums(const PointPass& pass, int fp64, int arith, hipStream_t st, int chunks, const PointSumsArgs& a) {
  if (bad_point_sums_launch(a, chunks) || bad_point_sums_queries(pass, a)) return (int)hipErrorInvalidValue;
  if (fp64) {   // fp64 contexts have one d2 form: REFERENCE = FMA3, REFERENCE_STRICT = STRICT
    if (arith & kStrict) launch_sums_one<P, double, d4, kStrict>(st, chunks, a);
    else launch_sums_one<P, double, d4, 0>(st, chunks, a);
  } else {
    switch (arith) {
      case NBODY_ARITH_REFERENCE: launch_sums_one<P, float, f4, kRef>(st, chunks, a); break;
      case NBODY_ARITH_STRICT: launch_sums_one<P, float, f4, kStrict>(st, chunks, a); break;
      case NBODY_ARITH_REFERENCE_STRICT: launch_sums_one<P, float, f4, kRef | kStrict>(st, chunks, a); break;
      default: launch_sums_one<P, float, f4, 0>(st, chunks, a); break;
    }
  }
  return (int)hipGetLastError();
}

template <class P>
int launch_combine(int fp64, hipStream_t st, const PointSumsArgs& a) {
  if (bad_point_sums_combine(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes);
  if (fp64) hipLaunchKernelGGL((block_sums_combine<P, double, d4>), grid, dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((block_sums_combine<P, float, f4>), grid, dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace

namespace nbl {

NBP_HIDDEN int launch_point_sums_kernel(const PointPass& pass, int fp64, int arith, hipStream_t st, int chunks, const PointSumsArgs& a) {
  if (pass.id == kSnapPass.id) return launch_sums<SnapSums>(pass, fp64, arith, st, chunks, a);
  if (pass.id == kJerkPass.id) return launch_sums<JerkSums>(pass, fp64, arith, st, chunks, a);
  return pass.id == kTidalPass.id ? launch_sums<TidalSums>(pass, fp64, arith, st, chunks, a) : launch_sums<FieldSums>(pass, fp64, arith, st, chunks, a);
}

NBP_HIDDEN int launch_point_sums_combine_kernel(const PointPass& pass, int fp64, hipStream_t st, const PointSumsArgs& a) {
  if (pass.id == kSnapPass.id) return launch_combine<SnapSums>(fp64, st, a);
  if (pass.id == kJerkPass.id) return launch_combine<JerkSums>(fp64, st, a);
  return pass.id == kTidalPass.id ? launch_combine<TidalSums>(fp64, st, a) : launch_combine<FieldSums>(fp64, st, a);
}

}  // namespace nbl
