// timescale.hip — the pair time-scale pass's device code: per row the smallest pair crossing time squared |r_ij|^2 / |v_ij|^2 over the
// other N - 1 bodies on the device, the body that gives it and the smallest squared distance (timescale_args.hpp states the rule,
// include/nbody.h the definitions), the combine of a split launch and the fixed-order reduction of a device's rows to its best.
// Compiles on its own; device.hip puts it into the library's one code object after hist.hip.  Reads nbody_args.hpp (f4, d4, NB_CONST)
// and nothing else of the force path.  d2 is diag_pass.hpp's plain_d2, v2 the same three operations on the velocity differences, q
// their IEEE quotient: the file is compiled with contraction off, and the plain `/` is the correctly rounded division (v_div_scale,
// v_rcp, the v_fma refinement, v_div_fmas, v_div_fixup).  No LDS in the hot kernel, no atomics, no inline assembly.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "timescale_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbts;
using namespace nbd;

#define NBTS_HIDDEN __attribute__((visibility("hidden")))

namespace {

// what a lane carries: the ascending scan's state
template <typename T>
struct Scale { T tau2; int idx; T d2min; };

// what the pass makes of diag_pass.hpp's pair_walk
template <typename T, typename V4>
struct TimescalePass {
  using State = Scale<T>;
  static __device__ __forceinline__ State start() { return {inf_of<T>(), -1, inf_of<T>()}; }
  // the statement of record: one pair of the ascending scan that replaces on strict <.  CMP: the excluded body's (j == sk) d2 is a quiet
  // NaN (plain_d2), and so is its q, whatever v2 is: a NaN is below nothing.  q = +inf (v2 = 0 < d2, an overflowed d2) is not below +inf.
  template <bool CMP>
  static __device__ __forceinline__ void pair(const V4 p, const V4 u, const V4 me, const V4 mv, int j, int sk, State& c) {
    const T d2 = plain_d2<CMP, T, V4>(p, me, j, sk);
    const T v2 = plain_d2<T, V4>(u, mv);
    const T q = d2 / v2;
    const bool less = q < c.tau2;
    c.tau2 = less ? q : c.tau2;
    c.idx = less ? j : c.idx;
    c.d2min = min_of(c.d2min, d2);
  }
  static __device__ __forceinline__ void to_scratch(const TimescaleArgs& a, size_t w, const State& c) {
    ((T*)scratch_tau2(a))[w] = c.tau2;
    ((T*)scratch_d2(a, sizeof(T)))[w] = c.d2min;
    scratch_idx(a, sizeof(T))[w] = c.idx;
  }
  static __device__ __forceinline__ void to_outputs(const TimescaleArgs& a, int p, const State& c) {
    if (a.tau2) ((T*)a.tau2)[p] = c.tau2;
    if (a.idx) a.idx[p] = c.idx;
    if (a.d2min) ((T*)a.d2min)[p] = c.d2min;
  }
};

// the walk is diag_pass.hpp's pair_walk, shared with pair_energy.hip: one row per lane, both source streams as scalar loads
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) timescale_kernel(TimescaleArgs a) {
  pair_walk<V4, TimescalePass<T, V4>>(a);
}

// the chunks of a split launch in ascending order: strict < for both minima; one row per lane (a wave reads 64 consecutive values)
template <typename T>
__global__ void __launch_bounds__(kLanes) timescale_combine(TimescaleArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.m) return;
  const T* st = (const T*)scratch_tau2(a);
  const T* sd = (const T*)scratch_d2(a, sizeof(T));
  const int* si = scratch_idx(a, sizeof(T));
  Scale<T> c = {inf_of<T>(), -1, inf_of<T>()};
  for (int y = 0; y < a.chunks; ++y) {
    const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
    const T q = st[w], d2 = sd[w];
    if (q < c.tau2) { c.tau2 = q; c.idx = si[w]; }
    if (d2 < c.d2min) c.d2min = d2;
  }
  if (a.tau2) ((T*)a.tau2)[p] = c.tau2;
  if (a.idx) a.idx[p] = c.idx;
  if (a.d2min) ((T*)a.d2min)[p] = c.d2min;
}

// the best of a device's rows: lane t takes rows t, t + 256, ... ascending with strict <, lane 0 then the 256 lanes' bests by
// (tau2, row) and the smallest of their d2min.  One workgroup, no atomics.  The lowest row that reaches the smallest tau2 is i.
template <typename T>
__global__ void __launch_bounds__(kLanes) timescale_best(const T* tau2, const int* idx, const T* d2min, int rows, int first, BestScale* out) {
  __shared__ double sq[kLanes], sd[kLanes];
  __shared__ int sr[kLanes];
  const int t = (int)threadIdx.x;
  T best = inf_of<T>(), dmin = inf_of<T>();
  int row = -1;
  for (int r = t; r < rows; r += kLanes) {
    const T q = tau2[r], d = d2min[r];
    if (q < best) { best = q; row = r; }
    if (d < dmin) dmin = d;
  }
  sq[t] = (double)best;
  sd[t] = (double)dmin;
  sr[t] = row;
  __syncthreads();
  if (t != 0) return;
  double b = (double)inf_of<T>(), bd = (double)inf_of<T>();
  int br = -1;
  for (int q = 0; q < kLanes; ++q) {
    if (sr[q] >= 0 && (sq[q] < b || (sq[q] == b && sr[q] < br))) { b = sq[q]; br = sr[q]; }
    if (sd[q] < bd) bd = sd[q];
  }
  out->tau2 = b;
  out->d2min = bd;
  out->i = br < 0 ? -1 : first + br;
  out->j = br < 0 ? -1 : idx[br];
}

}  // namespace

namespace nbl {

NBTS_HIDDEN int launch_timescale_kernel(int fp64, hipStream_t st, const TimescaleArgs& a) {
  if (bad_timescale_launch(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes, a.chunks), block(kLanes);
  if (fp64) hipLaunchKernelGGL((timescale_kernel<double, d4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((timescale_kernel<float, f4>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

NBTS_HIDDEN int launch_timescale_combine_kernel(int fp64, hipStream_t st, const TimescaleArgs& a) {
  if (bad_combine(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes);
  if (fp64) hipLaunchKernelGGL((timescale_combine<double>), grid, dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((timescale_combine<float>), grid, dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBTS_HIDDEN int launch_timescale_best_kernel(int fp64, hipStream_t st, const void* tau2, const int* idx, const void* d2min, int rows, int first,
                                             BestScale* out) {
  if (bad_row_reduce(rows, out, tau2 && idx && d2min)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((timescale_best<double>), dim3(1), dim3(kLanes), 0, st, (const double*)tau2, idx, (const double*)d2min, rows, first, out);
  else hipLaunchKernelGGL((timescale_best<float>), dim3(1), dim3(kLanes), 0, st, (const float*)tau2, idx, (const float*)d2min, rows, first, out);
  return (int)hipGetLastError();
}

}  // namespace nbl
