// hermite_block.hip — the device code of the Hermite integrator's individual block time steps (include/nbody.h, "individual block time
// steps"; hermite_block_args.hpp states what a row carries): the scheduler around the jerk points pass of point_sums.hip, which does the
// all-pairs work and is not touched.  Five kernels: init (base, tick 0, first level), predict-to-tau (every own row from its base, and
// the tiles' active counts), next-time (a device's smallest next tick and how many rows reach it, one workgroup, exact integers),
// compact-and-gather (the ascending list of active rows and their queries) and correct-and-assign (the active rows alone).
// The predictor and the corrector are hermite_args.hpp's expressions with h and the coefficients per row.  Compiles on its own;
// device.hip puts it into the library's one code object after hermite.hip.  The file is compiled with contraction off: a product is
// fused only where fma_of is written.  Plain vector stores, no atomics, no inline assembly.  gfx950 only (wave64: 64-bit ballots).
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "hermite_block_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbh;
using namespace nbhb;
using namespace nbd;

#define NBHB_HIDDEN __attribute__((visibility("hidden")))

namespace {

constexpr int kWaves = kLanes / 64;

template <typename T> __device__ __forceinline__ T unit_of(const BlockArgs& a);
template <> __device__ __forceinline__ float unit_of<float>(const BlockArgs& a) { return a.unit; }
template <> __device__ __forceinline__ double unit_of<double>(const BlockArgs& a) { return a.unit_d; }

// h of row p at tau: the ticks since its base, below 2^23 + 1 and so exact in T, times the tick: one rounding
template <typename T>
__device__ __forceinline__ T step_of(const BlockArgs& a, int p) { return (T)(a.tau - a.t0[p]) * unit_of<T>(a); }

__device__ __forceinline__ bool reaches(const BlockArgs& a, int p) { return a.t0[p] + ticks_of(a.level[p], a.levels) == a.tau; }

template <typename V4>
__global__ void __launch_bounds__(kLanes) hermite_block_init(const BlockArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.rows) return;
  ((V4*)a.x0)[p] = ((const V4*)a.pos)[p];
  ((V4*)a.v0)[p] = ((const V4*)a.vel)[p];
  a.t0[p] = 0;
  a.level[p] = wanted_level(((const V4*)a.a0)[p], ((const V4*)a.j0)[p], a.eta2, a.lim, a.levels);
}

// row p predicted from its base to tau; both fourth values are the base's.  The tile's rows that reach tau are counted by ballots
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) hermite_block_predict(const BlockArgs a) {
  __shared__ int wave_count[kWaves];
  const int t = (int)threadIdx.x;
  const int p = (int)blockIdx.x * kLanes + t;
  const bool live = p < a.rows;
  if (live) {
    const Coefficients<T> c = coefficients_of(step_of<T>(a, p));
    const V4 x0 = ((const V4*)a.x0)[p], v0 = ((const V4*)a.v0)[p], a0 = ((const V4*)a.a0)[p], j0 = ((const V4*)a.j0)[p];
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
  const unsigned long long mask = __ballot(live && reaches(a, live ? p : 0));
  if ((t & 63) == 0) wave_count[t >> 6] = __popcll(mask);
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int w = 0; w < kWaves; ++w) s += wave_count[w];
    a.counts[blockIdx.x] = s;
  }
}

// a device's smallest next tick and the rows that reach it, in hermite_best's two-level form: lane t takes rows t, t + 256, ...,
// lane 0 then the 256 lanes' words.  Integers: any order gives the same word.  One workgroup, no atomics.
__global__ void __launch_bounds__(kLanes) hermite_block_next(const long long* t0, const int* level, int rows, int levels, NextTime* out) {
  __shared__ long long st[kLanes];
  __shared__ int sc[kLanes];
  const int t = (int)threadIdx.x;
  long long best = kNoTick;
  int count = 0;
  for (int r = t; r < rows; r += kLanes) {
    const long long next = t0[r] + ticks_of(level[r], levels);
    if (next < best) { best = next; count = 1; }
    else if (next == best) ++count;
  }
  st[t] = best;
  sc[t] = count;
  __syncthreads();
  if (t != 0) return;
  long long b = kNoTick;
  int n = 0;
  for (int q = 0; q < kLanes; ++q) {
    if (sc[q] == 0) continue;
    if (st[q] < b) { b = st[q]; n = sc[q]; }
    else if (st[q] == b) n += sc[q];
  }
  out->tick = b;
  out->count = n;
  out->pad = 0;
}

// The active rows of the sub-step in ASCENDING order: tile b's rows go behind those of tiles 0 .. b - 1 (the counts predict left,
// summed by the workgroup's lanes), wave w's behind those of the tile's waves before it, lane l's behind the wave's lower lanes
// (the ballot's lower bits).  Ascending order keeps the skip indices of a wave of the jerk kernel close together (its
// wave_skip_window); the results cannot show the order — every query is evaluated alone and corrected into its own row — so no
// test checks it: the order is stated here.
template <typename V4>
__global__ void __launch_bounds__(kLanes) hermite_block_compact(const BlockArgs a) {
  __shared__ int part[kLanes];
  __shared__ int wave_count[kWaves];
  const int t = (int)threadIdx.x;
  const int p = (int)blockIdx.x * kLanes + t;
  int before = 0;
  for (int b = t; b < (int)blockIdx.x; b += kLanes) before += a.counts[b];
  part[t] = before;
  const bool act = p < a.rows && reaches(a, p < a.rows ? p : 0);
  const unsigned long long mask = __ballot(act);
  if ((t & 63) == 0) wave_count[t >> 6] = __popcll(mask);
  __syncthreads();
  if (!act) return;
  int at = 0;
  for (int q = 0; q < kLanes; ++q) at += part[q];
  for (int w = 0; w < (t >> 6); ++w) at += wave_count[w];
  at += __popcll(mask & ((1ull << (t & 63)) - 1ull));
  if (at >= a.m) return;   // (cannot happen: m is the sum of the counts; a store never leaves the buffers all the same)
  a.active[at] = p;
  ((V4*)a.q_points)[at] = ((const V4*)a.pos)[p];
  ((V4*)a.q_vel)[at] = ((const V4*)a.vel)[p];
  a.q_skip[at] = a.first + p;
}

// active row q of the list, row p of the slice: (x1, v1) from its base and the two evaluations with its own h; the base moves to tau
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) hermite_block_correct(const BlockArgs a) {
  const int q = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (q >= a.m) return;
  const int p = a.active[q];
  const Coefficients<T> c = coefficients_of(step_of<T>(a, p));
  const V4 x0 = ((const V4*)a.x0)[p], v0 = ((const V4*)a.v0)[p];
  const V4 a0 = ((const V4*)a.a0)[p], j0 = ((const V4*)a.j0)[p], a1 = ((const V4*)a.a1)[q], j1 = ((const V4*)a.j1)[q];
  V4 x1 = x0, v1 = v0;
  v1.x = fma_of(c.c12, j0.x - j1.x, fma_of(c.hh, a0.x + a1.x, v0.x));
  v1.y = fma_of(c.c12, j0.y - j1.y, fma_of(c.hh, a0.y + a1.y, v0.y));
  v1.z = fma_of(c.c12, j0.z - j1.z, fma_of(c.hh, a0.z + a1.z, v0.z));
  x1.x = fma_of(c.c12, a0.x - a1.x, fma_of(c.hh, v0.x + v1.x, x0.x));
  x1.y = fma_of(c.c12, a0.y - a1.y, fma_of(c.hh, v0.y + v1.y, x0.y));
  x1.z = fma_of(c.c12, a0.z - a1.z, fma_of(c.hh, v0.z + v1.z, x0.z));
  ((V4*)a.x0)[p] = x1;
  ((V4*)a.v0)[p] = v1;
  ((V4*)a.a0)[p] = a1;
  ((V4*)a.j0)[p] = j1;
  ((V4*)a.pos)[p] = x1;
  ((V4*)a.vel)[p] = v1;
  a.t0[p] = a.tau;
  a.level[p] = next_level(a.level[p], wanted_level(a1, j1, a.eta2, a.lim, a.levels), a.tau, a.levels);
}

inline dim3 tiles_of(int n) { return dim3((n + kLanes - 1) / kLanes); }

}  // namespace

namespace nbl {

NBHB_HIDDEN int launch_hermite_block_init_kernel(int fp64, hipStream_t st, const BlockArgs& a) {
  if (bad_block_rows(a)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite_block_init<d4>), tiles_of(a.rows), dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((hermite_block_init<f4>), tiles_of(a.rows), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBHB_HIDDEN int launch_hermite_block_predict_kernel(int fp64, hipStream_t st, const BlockArgs& a) {
  if (bad_block_predict(a)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite_block_predict<double, d4>), tiles_of(a.rows), dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((hermite_block_predict<float, f4>), tiles_of(a.rows), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBHB_HIDDEN int launch_hermite_block_next_kernel(hipStream_t st, const long long* t0, const int* level, int rows, int levels, NextTime* out) {
  if (bad_row_reduce(rows, out, t0 && level) || levels < 1 || levels > kMaxLevels) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(hermite_block_next, dim3(1), dim3(kLanes), 0, st, t0, level, rows, levels, out);
  return (int)hipGetLastError();
}

NBHB_HIDDEN int launch_hermite_block_compact_kernel(int fp64, hipStream_t st, const BlockArgs& a) {
  if (bad_block_compact(a)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite_block_compact<d4>), tiles_of(a.rows), dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((hermite_block_compact<f4>), tiles_of(a.rows), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBHB_HIDDEN int launch_hermite_block_correct_kernel(int fp64, hipStream_t st, const BlockArgs& a) {
  if (bad_block_correct(a)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite_block_correct<double, d4>), tiles_of(a.m), dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((hermite_block_correct<float, f4>), tiles_of(a.m), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
