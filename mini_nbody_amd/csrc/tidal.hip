// tidal.hip — the tidal pass's device code: the tidal tensor T = grad a = -grad grad phi of the N bodies on the device at m arbitrary
// points (tidal_args.hpp states the order, include/nbody.h the definitions).  Compiles on its own; device.hip puts it into the library's
// one code object after field.hip, whose shape it follows.  Reads nbody_args.hpp (f4, d4, NB_CONST) and nothing else of the force path:
// d2 and 1/sqrt are diag_pass.hpp's inv_dist, the potential's.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "tidal_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbt;
using namespace nbd;

#define NBT_HIDDEN __attribute__((visibility("hidden")))

namespace {

// the seven level-1 accumulators of one point
template <typename T>
struct TidalAcc { T xx, yy, zz, xy, xz, yz, s3; };

// one pair: 3 sub, d2, 1/sqrt, 3 mul (inv2, inv3, inv5), 1 mul (w = 3 inv5), 3 mul (w d), 6 fma, 1 add: 21 VALU + 1 transcendental in the
// fp32 timed form.  CMP: source j == sk keeps all seven accumulators as they are
template <int ARITH, bool CMP, typename T, typename V4>
__device__ __forceinline__ void tidal_pair(const V4 p, const V4 me, T eps, int j, int sk, TidalAcc<T>& c) {
  const T dx = p.x - me.x, dy = p.y - me.y, dz = p.z - me.z;
  const T inv = inv_dist<ARITH>(dx, dy, dz, eps);
  const T inv2 = inv * inv;
  const T inv3 = inv * inv2;
  const T inv5 = inv3 * inv2;
  const T w = (T)3 * inv5;
  const T wx = w * dx, wy = w * dy, wz = w * dz;
  const T xx = fma_of(wx, dx, c.xx), yy = fma_of(wy, dy, c.yy), zz = fma_of(wz, dz, c.zz);
  const T xy = fma_of(wx, dy, c.xy), xz = fma_of(wx, dz, c.xz), yz = fma_of(wy, dz, c.yz);
  const T s3 = c.s3 + inv3;
  if (CMP && j == sk) return;
  c.xx = xx; c.yy = yy; c.zz = zz; c.xy = xy; c.xz = xz; c.yz = yz; c.s3 = s3;
}

// the six values of point p from its level-2 sums l2 = {Qxx, Qyy, Qzz, Qxy, Qxz, Qyz, S3}: the diagonal's subtraction in fp64, rounded once
template <typename T>
__device__ __forceinline__ void tidal_store(const TidalArgs& a, int p, const double (&l2)[kSums]) {
  T* out = (T*)a.tensor + (size_t)p * kOut;
  out[0] = (T)(l2[0] - l2[6]); out[1] = (T)(l2[1] - l2[6]); out[2] = (T)(l2[2] - l2[6]);
  out[3] = (T)l2[3]; out[4] = (T)l2[4]; out[5] = (T)l2[5];
}

// One point per lane, kLanes points per workgroup; workgroup (x, y) walks the blocks of chunk y for the points of x, as field_kernel
// does: sources by wave-uniform scalar loads, lanes beyond m clamped to the last point and storing nothing, and with SKIP only the
// aligned 64-source windows that overlap the wave's [lowest, highest] skip index compare j with skip.
template <typename T, typename V4, int ARITH, bool SKIP>
__global__ void __launch_bounds__(kLanes) tidal_kernel(TidalArgs a) {
  const auto [p, live, pc] = lane_of(a.m);
  const V4 me = ((const V4*)a.points)[pc];
  const auto [sk, wlo, whi] = wave_skip_window<SKIP>(SKIP ? a.skip[pc] : -1);
  const T eps = soft<T>();
  const NB_CONST V4* src = scalar_src<V4>(a.src);
  T* sc = (T*)a.scratch;
  const auto [blk0, blk1] = chunk_of(a.chunk_blocks, a.n_blocks);
  double l2[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int blk = blk0; blk < blk1; ++blk) {
    const int b0 = blk * kSrcBlock;
    const int b1 = min(b0 + kSrcBlock, a.n_src);
    TidalAcc<T> c = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
    int j = b0;
    for (; j + 64 <= b1; j += 64) {
      if (!SKIP || j + 63 < wlo || j > whi) {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) tidal_pair<ARITH, false, T, V4>(src[j + k], me, eps, j + k, sk, c);
      } else {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) tidal_pair<ARITH, true, T, V4>(src[j + k], me, eps, j + k, sk, c);
      }
    }
    for (; j < b1; ++j) tidal_pair<ARITH, SKIP, T, V4>(src[j], me, eps, j, sk, c);   // the last block's tail (N not a multiple of 64)
    const T s[kSums] = {c.xx, c.yy, c.zz, c.xy, c.xz, c.yz, c.s3};
    if (sc) {
      if (live) {
        const size_t w = (size_t)blk * kSums * (size_t)a.m + (size_t)p;
#pragma unroll
        for (int q = 0; q < kSums; ++q) sc[w + (size_t)q * (size_t)a.m] = s[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < kSums; ++q) l2[q] += (double)s[q];
    }
  }
  if (!sc && live) tidal_store<T>(a, p, l2);
}

// level 2 from the stored per-block sums: blocks ascending, fp64, one point per lane (a wave reads 64 consecutive values per word)
template <typename T>
__global__ void __launch_bounds__(kLanes) tidal_combine(TidalArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.m) return;
  const T* sc = (const T*)a.scratch;
  const size_t m = (size_t)a.m;
  double l2[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int blk = 0; blk < a.n_blocks; ++blk) {
    const size_t w = (size_t)blk * kSums * m + (size_t)p;
#pragma unroll
    for (int q = 0; q < kSums; ++q) l2[q] += (double)sc[w + (size_t)q * m];
  }
  tidal_store<T>(a, p, l2);
}

template <typename T, typename V4, int ARITH>
void launch_tidal_one(hipStream_t st, int chunks, const TidalArgs& a) {
  const dim3 grid((a.m + kLanes - 1) / kLanes, chunks);
  if (a.skip) hipLaunchKernelGGL((tidal_kernel<T, V4, ARITH, true>), grid, dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((tidal_kernel<T, V4, ARITH, false>), grid, dim3(kLanes), 0, st, a);
}

}  // namespace

namespace nbl {

NBT_HIDDEN int launch_tidal_kernel(int fp64, int arith, hipStream_t st, int chunks, const TidalArgs& a) {
  if (a.m <= 0 || chunks < 1 || (chunks > 1 && !a.scratch) || !a.tensor) return (int)hipErrorInvalidValue;
  if (fp64) {   // fp64 contexts have one d2 form: REFERENCE = FMA3, REFERENCE_STRICT = STRICT
    if (arith & kStrict) launch_tidal_one<double, d4, kStrict>(st, chunks, a);
    else launch_tidal_one<double, d4, 0>(st, chunks, a);
  } else {
    switch (arith) {
      case NBODY_ARITH_REFERENCE: launch_tidal_one<float, f4, kRef>(st, chunks, a); break;
      case NBODY_ARITH_STRICT: launch_tidal_one<float, f4, kStrict>(st, chunks, a); break;
      case NBODY_ARITH_REFERENCE_STRICT: launch_tidal_one<float, f4, kRef | kStrict>(st, chunks, a); break;
      default: launch_tidal_one<float, f4, 0>(st, chunks, a); break;
    }
  }
  return (int)hipGetLastError();
}

NBT_HIDDEN int launch_tidal_combine_kernel(int fp64, hipStream_t st, const TidalArgs& a) {
  if (a.m <= 0 || !a.scratch || !a.tensor) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes);
  if (fp64) hipLaunchKernelGGL((tidal_combine<double>), grid, dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((tidal_combine<float>), grid, dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
