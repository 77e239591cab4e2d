// pair_energy.hip — the pair binding-energy pass's device code: per row the lowest specific two-body energy v2 / 2 - 2 / sqrt(d2 + eps)
// over the other N - 1 bodies on the device and the body that gives it (pair_energy_args.hpp states the rule, include/nbody.h the
// definitions), and the combine of a split launch.  Compiles on its own; device.hip puts it into the library's one code object after
// timescale.hip.  Reads nbody_args.hpp (f4, d4, NB_CONST, kSoftBits) and nothing else of the force path.  d2 is diag_pass.hpp's
// plain_d2, v2 the same three operations on the velocity differences, the walk diag_pass.hpp's pair_walk, which timescale.hip shares.
// The file is compiled with contraction off: the one fma of e is the one the source names.  binary32: 1 / sqrt is the expression
// inv_dist uses under a strict mode, evaluated as written — the correctly rounded binary64 sqrt and quotient, then one conversion.
// No LDS, no atomics, no inline assembly.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "pair_energy_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbpe;
using namespace nbd;

#define NBPE_HIDDEN __attribute__((visibility("hidden")))

namespace {

// what a lane carries: the ascending scan's state
template <typename T>
struct Bound { T e; int idx; };

// (d2 + eps)^(-1/2), one definition per precision whatever NBODY_OPT_ARITH says
__device__ __forceinline__ float inv_soft(float s) { return (float)(1.0 / __builtin_sqrt((double)s)); }
__device__ __forceinline__ double inv_soft(double s) { return 1.0 / __builtin_sqrt(s); }

// what the pass makes of diag_pass.hpp's pair_walk
template <typename T, typename V4>
struct PairEnergyPass {
  using State = Bound<T>;
  static __device__ __forceinline__ State start() { return {inf_of<T>(), -1}; }
  // the statement of record: one pair of the ascending scan that replaces on strict <.  CMP: the excluded body's (j == sk) d2 is a quiet
  // NaN (plain_d2), and so are its s, inv and e: a NaN is below nothing.  e = +inf (an overflowed v2) is not below +inf; an overflowed
  // d2 gives inv = +0 and e = v2 / 2.
  template <bool CMP>
  static __device__ __forceinline__ void pair(const V4 p, const V4 u, const V4 me, const V4 mv, int j, int sk, State& c) {
    const T d2 = plain_d2<CMP, T, V4>(p, me, j, sk);
    const T v2 = plain_d2<T, V4>(u, mv);
    const T inv = inv_soft(d2 + soft<T>());
    const T e = fma_of((T)0.5, v2, (T)-2 * inv);
    const bool less = e < c.e;
    c.e = less ? e : c.e;
    c.idx = less ? j : c.idx;
  }
  static __device__ __forceinline__ void to_scratch(const PairEnergyArgs& a, size_t w, const State& c) {
    ((T*)scratch_e(a))[w] = c.e;
    scratch_idx(a, sizeof(T))[w] = c.idx;
  }
  static __device__ __forceinline__ void to_outputs(const PairEnergyArgs& a, int p, const State& c) {
    if (a.e) ((T*)a.e)[p] = c.e;
    if (a.idx) a.idx[p] = c.idx;
  }
};

template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) pair_energy_kernel(PairEnergyArgs a) {
  pair_walk<V4, PairEnergyPass<T, V4>>(a);
}

// the chunks of a split launch in ascending order with strict <; one row per lane (a wave reads 64 consecutive values)
template <typename T>
__global__ void __launch_bounds__(kLanes) pair_energy_combine(PairEnergyArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.m) return;
  const T* se = (const T*)scratch_e(a);
  const int* si = scratch_idx(a, sizeof(T));
  Bound<T> c = {inf_of<T>(), -1};
  for (int y = 0; y < a.chunks; ++y) {
    const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
    const T e = se[w];
    if (e < c.e) { c.e = e; c.idx = si[w]; }
  }
  if (a.e) ((T*)a.e)[p] = c.e;
  if (a.idx) a.idx[p] = c.idx;
}

}  // namespace

namespace nbl {

NBPE_HIDDEN int launch_pair_energy_kernel(int fp64, hipStream_t st, const PairEnergyArgs& a) {
  if (bad_pair_energy_launch(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes, a.chunks), block(kLanes);
  if (fp64) hipLaunchKernelGGL((pair_energy_kernel<double, d4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((pair_energy_kernel<float, f4>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

NBPE_HIDDEN int launch_pair_energy_combine_kernel(int fp64, hipStream_t st, const PairEnergyArgs& a) {
  if (bad_pair_energy_combine(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes);
  if (fp64) hipLaunchKernelGGL((pair_energy_combine<double>), grid, dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((pair_energy_combine<float>), grid, dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
