// hermite6.hip — the sixth-order Hermite step's device code beside the snap pass (point_sums.hip, which does the all-pairs work): the
// predictor and the corrector with the crackle of the next predictor, one row per lane (hermite6_args.hpp states the arithmetic,
// include/nbody.h the scheme).  The best-row reduction is hermite.hip's.  Compiles on its own; device.hip puts it into the library's one
// code object after hermite_block.hip.  Reads nbody_args.hpp (f4, d4) and nothing else of the force path.  The file is compiled with
// contraction off: a product is fused only where fma_of is written.  Plain vector stores, no atomics, no inline assembly.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "hermite6_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbh6;
using namespace nbd;

#define NBH6_HIDDEN __attribute__((visibility("hidden")))

namespace {

template <typename T> __device__ __forceinline__ const Coefficients6<T>& coefficients6(const Hermite6Args& a);
template <> __device__ __forceinline__ const Coefficients6<float>& coefficients6<float>(const Hermite6Args& a) { return a.f; }
template <> __device__ __forceinline__ const Coefficients6<double>& coefficients6<double>(const Hermite6Args& a) { return a.d; }

// one component of the three Taylor sums
template <typename T>
__device__ __forceinline__ T predict_x(const Coefficients6<T>& c, T x0, T v0, T a0, T j0, T s0, T c0) {
  return fma_of(c.c5, c0, fma_of(c.c4, s0, fma_of(c.c3, j0, fma_of(c.c2, a0, fma_of(c.h, v0, x0)))));
}
template <typename T>
__device__ __forceinline__ T predict_v(const Coefficients6<T>& c, T v0, T a0, T j0, T s0, T c0) {
  return fma_of(c.c4, c0, fma_of(c.c3, s0, fma_of(c.c2, j0, fma_of(c.h, a0, v0))));
}
template <typename T>
__device__ __forceinline__ T predict_a(const Coefficients6<T>& c, T a0, T j0, T s0, T c0) {
  return fma_of(c.c3, c0, fma_of(c.c2, s0, fma_of(c.h, j0, a0)));
}

// row p: (x0, v0) saved aside, the predicted (xp, vp) in their place and ap beside them; the fourth values stay
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) hermite6_predict(const Hermite6Args a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.rows) return;
  const Coefficients6<T> c = coefficients6<T>(a);
  const V4 x0 = ((const V4*)a.pos)[p], v0 = ((const V4*)a.vel)[p];
  const V4 a0 = ((const V4*)a.a0)[p], j0 = ((const V4*)a.j0)[p], s0 = ((const V4*)a.s0)[p], c0 = ((const V4*)a.crk)[p];
  ((V4*)a.pos0)[p] = x0;
  ((V4*)a.vel0)[p] = v0;
  V4 xp = x0, vp = v0, ap = a0;
  xp.x = predict_x(c, x0.x, v0.x, a0.x, j0.x, s0.x, c0.x);
  xp.y = predict_x(c, x0.y, v0.y, a0.y, j0.y, s0.y, c0.y);
  xp.z = predict_x(c, x0.z, v0.z, a0.z, j0.z, s0.z, c0.z);
  vp.x = predict_v(c, v0.x, a0.x, j0.x, s0.x, c0.x);
  vp.y = predict_v(c, v0.y, a0.y, j0.y, s0.y, c0.y);
  vp.z = predict_v(c, v0.z, a0.z, j0.z, s0.z, c0.z);
  ap.x = predict_a(c, a0.x, j0.x, s0.x, c0.x);
  ap.y = predict_a(c, a0.y, j0.y, s0.y, c0.y);
  ap.z = predict_a(c, a0.z, j0.z, s0.z, c0.z);
  ((V4*)a.pos)[p] = xp;
  ((V4*)a.vel)[p] = vp;
  ((V4*)a.ap)[p] = ap;
}

// one component of the corrector: v1, then x1 with it, and the crackle at the end of the step
template <typename T>
struct Corrected { T x1, v1, c1; };
template <typename T>
__device__ __forceinline__ Corrected<T> correct_one(const Coefficients6<T>& c, T x0, T v0, T a0, T j0, T s0, T a1, T j1, T s1) {
  const T v1 = fma_of(c.c120, s0 + s1, fma_of(c.c10, j0 - j1, fma_of(c.hh, a0 + a1, v0)));
  const T x1 = fma_of(c.c120, j0 + j1, fma_of(c.c10, a0 - a1, fma_of(c.hh, v0 + v1, x0)));
  const T e1 = (T)60 * (a1 - a0);
  const T e2 = fma_of((T)36, j1, (T)24 * j0);
  const T e3 = fma_of((T)9, s1, (T)-3 * s0);
  return {x1, v1, c.r * fma_of(c.r, fma_of(c.r, e1, -e2), e3)};
}

// row p: (x1, v1) from the saved (x0, v0) and the two evaluations, c1 for the next predictor; the fourth values of the state are the
// saved words', that of c1 is a1's
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) hermite6_correct(const Hermite6Args a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.rows) return;
  const Coefficients6<T> c = coefficients6<T>(a);
  const V4 x0 = ((const V4*)a.pos0)[p], v0 = ((const V4*)a.vel0)[p];
  const V4 a0 = ((const V4*)a.a0)[p], j0 = ((const V4*)a.j0)[p], s0 = ((const V4*)a.s0)[p];
  const V4 a1 = ((const V4*)a.a1)[p], j1 = ((const V4*)a.j1)[p], s1 = ((const V4*)a.s1)[p];
  V4 x1 = x0, v1 = v0, c1 = a1;
  const Corrected<T> rx = correct_one(c, x0.x, v0.x, a0.x, j0.x, s0.x, a1.x, j1.x, s1.x);
  const Corrected<T> ry = correct_one(c, x0.y, v0.y, a0.y, j0.y, s0.y, a1.y, j1.y, s1.y);
  const Corrected<T> rz = correct_one(c, x0.z, v0.z, a0.z, j0.z, s0.z, a1.z, j1.z, s1.z);
  x1.x = rx.x1; x1.y = ry.x1; x1.z = rz.x1;
  v1.x = rx.v1; v1.y = ry.v1; v1.z = rz.v1;
  c1.x = rx.c1; c1.y = ry.c1; c1.z = rz.c1;
  ((V4*)a.pos)[p] = x1;
  ((V4*)a.vel)[p] = v1;
  ((V4*)a.crk)[p] = c1;
}

}  // namespace

namespace nbl {

NBH6_HIDDEN int launch_hermite6_predict_kernel(int fp64, hipStream_t st, const Hermite6Args& a) {
  if (bad_hermite6_predict(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.rows + kLanes - 1) / kLanes), block(kLanes);
  if (fp64) hipLaunchKernelGGL((hermite6_predict<double, d4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((hermite6_predict<float, f4>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

NBH6_HIDDEN int launch_hermite6_correct_kernel(int fp64, hipStream_t st, const Hermite6Args& a) {
  if (bad_hermite6_correct(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.rows + kLanes - 1) / kLanes), block(kLanes);
  if (fp64) hipLaunchKernelGGL((hermite6_correct<double, d4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((hermite6_correct<float, f4>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
