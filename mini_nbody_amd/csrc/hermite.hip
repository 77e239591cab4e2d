// hermite.hip — the Hermite step's device code beside the jerk pass (point_sums.hip, which does the all-pairs work and is not touched):
// the predictor and the corrector, one row per lane, and the fixed-order reduction of a device's rows to its smallest |a|^2 / |j|^2
// (hermite_args.hpp states the arithmetic, include/nbody.h the scheme).  Compiles on its own; device.hip puts it into the library's one
// code object after timescale.hip.  Reads nbody_args.hpp (f4, d4) and nothing else of the force path.  The file is compiled with
// contraction off: a product is fused only where fma_of is written.  Plain vector stores, no atomics, no inline assembly.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "hermite_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbh;
using namespace nbd;

#define NBH_HIDDEN __attribute__((visibility("hidden")))

namespace {

template <typename T> __device__ __forceinline__ Coefficients<T> coefficients(const HermiteArgs& a);
template <> __device__ __forceinline__ Coefficients<float> coefficients<float>(const HermiteArgs& a) { return {a.h, a.c2, a.c3, a.hh, a.c12}; }
template <> __device__ __forceinline__ Coefficients<double> coefficients<double>(const HermiteArgs& a) { return {a.h_d, a.c2_d, a.c3_d, a.hh_d, a.c12_d}; }

// row p: (x0, v0) saved aside, the predicted (xp, vp) in their place; both fourth values stay
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) hermite_predict(const HermiteArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.rows) return;
  const Coefficients<T> c = coefficients<T>(a);
  const V4 x0 = ((const V4*)a.pos)[p], v0 = ((const V4*)a.vel)[p], a0 = ((const V4*)a.a0)[p], j0 = ((const V4*)a.j0)[p];
  ((V4*)a.pos0)[p] = x0;
  ((V4*)a.vel0)[p] = v0;
  V4 xp = x0, vp = v0;
  xp.x = fma_of(c.c3, j0.x, fma_of(c.c2, a0.x, fma_of(c.h, v0.x, x0.x)));
  xp.y = fma_of(c.c3, j0.y, fma_of(c.c2, a0.y, fma_of(c.h, v0.y, x0.y)));
  xp.z = fma_of(c.c3, j0.z, fma_of(c.c2, a0.z, fma_of(c.h, v0.z, x0.z)));
  vp.x = fma_of(c.c2, j0.x, fma_of(c.h, a0.x, v0.x));
  vp.y = fma_of(c.c2, j0.y, fma_of(c.h, a0.y, v0.y));
  vp.z = fma_of(c.c2, j0.z, fma_of(c.h, a0.z, v0.z));
  ((V4*)a.pos)[p] = xp;
  ((V4*)a.vel)[p] = vp;
}

// row p: (x1, v1) from the saved (x0, v0) and the two evaluations; both fourth values are the saved words'
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) hermite_correct(const HermiteArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.rows) return;
  const Coefficients<T> c = coefficients<T>(a);
  const V4 x0 = ((const V4*)a.pos0)[p], v0 = ((const V4*)a.vel0)[p];
  const V4 a0 = ((const V4*)a.a0)[p], j0 = ((const V4*)a.j0)[p], a1 = ((const V4*)a.a1)[p], j1 = ((const V4*)a.j1)[p];
  V4 x1 = x0, v1 = v0;
  v1.x = fma_of(c.c12, j0.x - j1.x, fma_of(c.hh, a0.x + a1.x, v0.x));
  v1.y = fma_of(c.c12, j0.y - j1.y, fma_of(c.hh, a0.y + a1.y, v0.y));
  v1.z = fma_of(c.c12, j0.z - j1.z, fma_of(c.hh, a0.z + a1.z, v0.z));
  x1.x = fma_of(c.c12, a0.x - a1.x, fma_of(c.hh, v0.x + v1.x, x0.x));
  x1.y = fma_of(c.c12, a0.y - a1.y, fma_of(c.hh, v0.y + v1.y, x0.y));
  x1.z = fma_of(c.c12, a0.z - a1.z, fma_of(c.hh, v0.z + v1.z, x0.z));
  ((V4*)a.pos)[p] = x1;
  ((V4*)a.vel)[p] = v1;
}

// the best of a device's rows, in timescale_best's two-level form: lane t takes rows t, t + 256, ... ascending with strict < from +inf (q = ratio_of, hermite_args.hpp)
// (a NaN or +inf q is below nothing), lane 0 then the 256 lanes' bests by (q, row).  One workgroup, no atomics.
template <typename V4>
__global__ void __launch_bounds__(kLanes) hermite_best(const V4* accel, const V4* jerk, int rows, int first, BestRatio* out) {
  __shared__ double sq[kLanes];
  __shared__ int sr[kLanes];
  const int t = (int)threadIdx.x;
  double best = (double)inf_of<float>();
  int row = -1;
  for (int r = t; r < rows; r += kLanes) {
    const double q = ratio_of(accel[r], jerk[r]);
    if (q < best) { best = q; row = r; }
  }
  sq[t] = best;
  sr[t] = row;
  __syncthreads();
  if (t != 0) return;
  double b = (double)inf_of<float>();
  int br = -1;
  for (int q = 0; q < kLanes; ++q)
    if (sr[q] >= 0 && (sq[q] < b || (sq[q] == b && sr[q] < br))) { b = sq[q]; br = sr[q]; }
  out->q = b;
  out->row = br < 0 ? -1 : first + br;
  out->pad = 0;
}

}  // namespace

namespace nbl {

NBH_HIDDEN int launch_hermite_predict_kernel(int fp64, hipStream_t st, const HermiteArgs& a) {
  if (bad_hermite_predict(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.rows + kLanes - 1) / kLanes), block(kLanes);
  if (fp64) hipLaunchKernelGGL((hermite_predict<double, d4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((hermite_predict<float, f4>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

NBH_HIDDEN int launch_hermite_correct_kernel(int fp64, hipStream_t st, const HermiteArgs& a) {
  if (bad_hermite_correct(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.rows + kLanes - 1) / kLanes), block(kLanes);
  if (fp64) hipLaunchKernelGGL((hermite_correct<double, d4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((hermite_correct<float, f4>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

NBH_HIDDEN int launch_hermite_best_kernel(int fp64, hipStream_t st, const void* accel, const void* jerk, int rows, int first, BestRatio* out) {
  if (bad_row_reduce(rows, out, accel && jerk)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite_best<d4>), dim3(1), dim3(kLanes), 0, st, (const d4*)accel, (const d4*)jerk, rows, first, out);
  else hipLaunchKernelGGL((hermite_best<f4>), dim3(1), dim3(kLanes), 0, st, (const f4*)accel, (const f4*)jerk, rows, first, out);
  return (int)hipGetLastError();
}

}  // namespace nbl
