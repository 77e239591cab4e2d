// field.hip — the field pass's device code: acceleration and potential of the N bodies on the device at m arbitrary points
// (field_args.hpp states the order, include/nbody.h the definitions).  Compiles on its own; device.hip puts it into the library's one
// code object after kernels.hip and energy.hip.  Reads nbody_args.hpp (f4, d4, NB_CONST) and nothing else of the force path: d2 and
// 1/sqrt are diag_pass.hpp's inv_dist, the potential's; the cube and the three fma follow the force's pair_f32 / pair_f64.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "field_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbf;
using namespace nbd;

#define NBF_HIDDEN __attribute__((visibility("hidden")))

namespace {

// the four level-1 accumulators of one point
template <typename T>
struct Acc { T ax, ay, az, s; };

// one pair: 3 sub, d2, 1/sqrt, 2 mul (the force's cube), 3 fma, 1 add.  CMP: source j == sk keeps all four accumulators as they are
template <int ARITH, bool CMP, typename T, typename V4>
__device__ __forceinline__ void pair(const V4 p, const V4 me, T eps, int j, int sk, Acc<T>& c) {
  const T dx = p.x - me.x, dy = p.y - me.y, dz = p.z - me.z;
  const T inv = inv_dist<ARITH>(dx, dy, dz, eps);
  const T inv2 = inv * inv;
  const T inv3 = inv * inv2;
  const T ax = fma_of(dx, inv3, c.ax), ay = fma_of(dy, inv3, c.ay), az = fma_of(dz, inv3, c.az), s = c.s + inv;
  if (CMP && j == sk) return;
  c.ax = ax; c.ay = ay; c.az = az; c.s = s;
}

template <typename T, typename V4>
__device__ __forceinline__ void store_out(const FieldArgs& a, int p, double ax, double ay, double az, double s) {
  if (a.accel) ((V4*)a.accel)[p] = V4{(T)ax, (T)ay, (T)az, (T)0};
  if (a.phi) ((T*)a.phi)[p] = (T)(0.0 - s);
}

// One point per lane, kLanes points per workgroup; workgroup (x, y) walks the blocks of chunk y for the points of x.  Sources
// arrive with wave-uniform scalar loads (address space 4, as energy_kernel).  Lanes beyond m stay in the wave-uniform loops clamped to
// the last point and store nothing.  SKIP: only the aligned 64-source windows that overlap [lowest, highest] skip index of the wave's
// 64 points compare j with skip (a wave-uniform branch); every other window, and every window of the SKIP = false form, is 3 sub,
// 3 fma, 1 rsq, 2 mul, 3 fma and 1 add per pair.
template <typename T, typename V4, int ARITH, bool SKIP>
__global__ void __launch_bounds__(kLanes) field_kernel(FieldArgs a) {
  const auto [p, live, pc] = lane_of(a.m);
  const V4 me = ((const V4*)a.points)[pc];
  const auto [sk, wlo, whi] = wave_skip_window<SKIP>(SKIP ? a.skip[pc] : -1);
  const T eps = soft<T>();
  const NB_CONST V4* src = scalar_src<V4>(a.src);
  T* sc = (T*)a.scratch;
  const auto [blk0, blk1] = chunk_of(a.chunk_blocks, a.n_blocks);
  double l2x = 0.0, l2y = 0.0, l2z = 0.0, l2s = 0.0;
  for (int blk = blk0; blk < blk1; ++blk) {
    const int b0 = blk * kSrcBlock;
    const int b1 = min(b0 + kSrcBlock, a.n_src);
    Acc<T> c = {(T)0, (T)0, (T)0, (T)0};
    int j = b0;
    for (; j + 64 <= b1; j += 64) {
      if (!SKIP || j + 63 < wlo || j > whi) {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) pair<ARITH, false, T, V4>(src[j + k], me, eps, j + k, sk, c);
      } else {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) pair<ARITH, true, T, V4>(src[j + k], me, eps, j + k, sk, c);
      }
    }
    for (; j < b1; ++j) pair<ARITH, SKIP, T, V4>(src[j], me, eps, j, sk, c);   // the last block's tail (N not a multiple of 64)
    if (sc) {
      if (live) {
        const size_t w = (size_t)blk * 4 * (size_t)a.m + (size_t)p;
        sc[w] = c.ax; sc[w + (size_t)a.m] = c.ay; sc[w + 2 * (size_t)a.m] = c.az; sc[w + 3 * (size_t)a.m] = c.s;
      }
    } else {
      l2x += (double)c.ax; l2y += (double)c.ay; l2z += (double)c.az; l2s += (double)c.s;
    }
  }
  if (!sc && live) store_out<T, V4>(a, p, l2x, l2y, l2z, l2s);
}

// level 2 from the stored per-block sums: blocks ascending, fp64, one point per lane (a wave reads 64 consecutive values per word)
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) field_combine(FieldArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.m) return;
  const T* sc = (const T*)a.scratch;
  const size_t m = (size_t)a.m;
  double l2x = 0.0, l2y = 0.0, l2z = 0.0, l2s = 0.0;
  for (int blk = 0; blk < a.n_blocks; ++blk) {
    const size_t w = (size_t)blk * 4 * m + (size_t)p;
    l2x += (double)sc[w]; l2y += (double)sc[w + m]; l2z += (double)sc[w + 2 * m]; l2s += (double)sc[w + 3 * m];
  }
  store_out<T, V4>(a, p, l2x, l2y, l2z, l2s);
}

template <typename T, typename V4, int ARITH>
void launch_field_one(hipStream_t st, int chunks, const FieldArgs& a) {
  const dim3 grid((a.m + kLanes - 1) / kLanes, chunks);
  if (a.skip) hipLaunchKernelGGL((field_kernel<T, V4, ARITH, true>), grid, dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((field_kernel<T, V4, ARITH, false>), grid, dim3(kLanes), 0, st, a);
}

}  // namespace

namespace nbl {

NBF_HIDDEN int launch_field_kernel(int fp64, int arith, hipStream_t st, int chunks, const FieldArgs& a) {
  if (a.m <= 0 || chunks < 1 || (chunks > 1 && !a.scratch)) return (int)hipErrorInvalidValue;
  if (fp64) {   // fp64 contexts have one d2 form: REFERENCE = FMA3, REFERENCE_STRICT = STRICT
    if (arith & kStrict) launch_field_one<double, d4, kStrict>(st, chunks, a);
    else launch_field_one<double, d4, 0>(st, chunks, a);
  } else {
    switch (arith) {
      case NBODY_ARITH_REFERENCE: launch_field_one<float, f4, kRef>(st, chunks, a); break;
      case NBODY_ARITH_STRICT: launch_field_one<float, f4, kStrict>(st, chunks, a); break;
      case NBODY_ARITH_REFERENCE_STRICT: launch_field_one<float, f4, kRef | kStrict>(st, chunks, a); break;
      default: launch_field_one<float, f4, 0>(st, chunks, a); break;
    }
  }
  return (int)hipGetLastError();
}

NBF_HIDDEN int launch_field_combine_kernel(int fp64, hipStream_t st, const FieldArgs& a) {
  if (a.m <= 0 || !a.scratch) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes);
  if (fp64) hipLaunchKernelGGL((field_combine<double, d4>), grid, dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((field_combine<float, f4>), grid, dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
