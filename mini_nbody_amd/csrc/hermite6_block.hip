// hermite6_block.hip — the device code of the sixth-order Hermite integrator's individual block time steps (include/nbody.h,
// "sixth-order individual block time steps"; hermite6_block_args.hpp states what a row carries): the scheduler around the snap points
// pass of point_sums.hip, which does the all-pairs work and is not touched.  Four kernels: init (base, tick 0, first level),
// predict-to-tau (every own row from its base: xp, vp and ap, and the tiles' active counts), compact-and-gather (the ascending list of
// active rows and their queries) and correct-and-assign (the active rows alone, with the crackle of their next predictor).  The
// next-time kernel is hermite_block.hip's.  The predictor and the corrector are hermite6_args.hpp's expressions with h and the
// coefficients per row (coefficients6_of on the device: products and correctly rounded quotients only).  Compiles on its own;
// device.hip puts it into the library's one code object after hermite6.hip.  The file is compiled with contraction off: a product is
// fused only where fma_of is written.  One row per lane, plain vector stores, no atomics, no inline assembly, no LDS beyond the tile
// counts.  gfx950 only (wave64: 64-bit ballots).
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "hermite6_block_args.hpp"
#include "nbody_args.hpp"

#define NBH6B_HIDDEN __attribute__((visibility("hidden")))

namespace {
namespace h6b {   // (device.hip compiles this file in one translation unit with hermite_block.hip and hermite6.hip: the names stay apart)

using namespace nbk;
using namespace nbh6;
using namespace nbh6b;
using namespace nbhb;
using namespace nbd;

constexpr int kWaves = kLanes / 64;

template <typename T> __device__ __forceinline__ T unit_of(const BlockArgs& a);
template <> __device__ __forceinline__ float unit_of<float>(const BlockArgs& a) { return a.unit; }
template <> __device__ __forceinline__ double unit_of<double>(const BlockArgs& a) { return a.unit_d; }

// h of row p at tau: the ticks since its base, below 2^23 + 1 and so exact in T, times the tick: one rounding
template <typename T>
__device__ __forceinline__ T step_of(const BlockArgs& a, int p) { return (T)(a.tau - a.t0[p]) * unit_of<T>(a); }

__device__ __forceinline__ bool reaches(const BlockArgs& a, int p) { return a.t0[p] + ticks_of(a.level[p], a.levels) == a.tau; }

template <typename V4>
__global__ void __launch_bounds__(kLanes) hermite6_block_init(const Block6Args a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.b.rows) return;
  ((V4*)a.b.x0)[p] = ((const V4*)a.b.pos)[p];
  ((V4*)a.b.v0)[p] = ((const V4*)a.b.vel)[p];
  a.b.t0[p] = 0;
  a.b.level[p] = wanted_level(((const V4*)a.b.a0)[p], ((const V4*)a.b.j0)[p], a.b.eta2, a.b.lim, a.b.levels);
}

// one component of the three Taylor sums (hermite6_args.hpp)
template <typename T>
__device__ __forceinline__ T taylor_x(const Coefficients6<T>& c, T x0, T v0, T a0, T j0, T s0, T c0) {
  return fma_of(c.c5, c0, fma_of(c.c4, s0, fma_of(c.c3, j0, fma_of(c.c2, a0, fma_of(c.h, v0, x0)))));
}
template <typename T>
__device__ __forceinline__ T taylor_v(const Coefficients6<T>& c, T v0, T a0, T j0, T s0, T c0) {
  return fma_of(c.c4, c0, fma_of(c.c3, s0, fma_of(c.c2, j0, fma_of(c.h, a0, v0))));
}
template <typename T>
__device__ __forceinline__ T taylor_a(const Coefficients6<T>& c, T a0, T j0, T s0, T c0) {
  return fma_of(c.c3, c0, fma_of(c.c2, s0, fma_of(c.h, j0, a0)));
}

// row p predicted from its base to tau; the fourth values are the base's (ap: a0's, 0).  The tile's rows that reach tau are counted
// by ballots
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) hermite6_block_predict(const Block6Args a) {
  __shared__ int wave_count[kWaves];
  const int t = (int)threadIdx.x;
  const int p = (int)blockIdx.x * kLanes + t;
  const bool live = p < a.b.rows;
  if (live) {
    const Coefficients6<T> c = coefficients6_of(step_of<T>(a.b, p));
    const V4 x0 = ((const V4*)a.b.x0)[p], v0 = ((const V4*)a.b.v0)[p], a0 = ((const V4*)a.b.a0)[p], j0 = ((const V4*)a.b.j0)[p];
    const V4 s0 = ((const V4*)a.s0)[p], c0 = ((const V4*)a.c0)[p];
    V4 xp = x0, vp = v0, ap = a0;
    xp.x = taylor_x(c, x0.x, v0.x, a0.x, j0.x, s0.x, c0.x);
    xp.y = taylor_x(c, x0.y, v0.y, a0.y, j0.y, s0.y, c0.y);
    xp.z = taylor_x(c, x0.z, v0.z, a0.z, j0.z, s0.z, c0.z);
    vp.x = taylor_v(c, v0.x, a0.x, j0.x, s0.x, c0.x);
    vp.y = taylor_v(c, v0.y, a0.y, j0.y, s0.y, c0.y);
    vp.z = taylor_v(c, v0.z, a0.z, j0.z, s0.z, c0.z);
    ap.x = taylor_a(c, a0.x, j0.x, s0.x, c0.x);
    ap.y = taylor_a(c, a0.y, j0.y, s0.y, c0.y);
    ap.z = taylor_a(c, a0.z, j0.z, s0.z, c0.z);
    ((V4*)a.b.pos)[p] = xp;
    ((V4*)a.b.vel)[p] = vp;
    ((V4*)a.ap)[p] = ap;
  }
  const unsigned long long mask = __ballot(live && reaches(a.b, live ? p : 0));
  if ((t & 63) == 0) wave_count[t >> 6] = __popcll(mask);
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int w = 0; w < kWaves; ++w) s += wave_count[w];
    a.b.counts[blockIdx.x] = s;
  }
}

// The active rows of the sub-step in ASCENDING order, as hermite_block.hip lists them: tile b's rows behind those of tiles 0 .. b - 1
// (the counts predict left), wave w's behind those of the tile's waves before it, lane l's behind the wave's lower lanes.  The results
// cannot show the order — every query is evaluated alone and corrected into its own row —: it is stated here.
template <typename V4>
__global__ void __launch_bounds__(kLanes) hermite6_block_compact(const Block6Args a) {
  __shared__ int part[kLanes];
  __shared__ int wave_count[kWaves];
  const int t = (int)threadIdx.x;
  const int p = (int)blockIdx.x * kLanes + t;
  int before = 0;
  for (int b = t; b < (int)blockIdx.x; b += kLanes) before += a.b.counts[b];
  part[t] = before;
  const bool act = p < a.b.rows && reaches(a.b, p < a.b.rows ? p : 0);
  const unsigned long long mask = __ballot(act);
  if ((t & 63) == 0) wave_count[t >> 6] = __popcll(mask);
  __syncthreads();
  if (!act) return;
  int at = 0;
  for (int q = 0; q < kLanes; ++q) at += part[q];
  for (int w = 0; w < (t >> 6); ++w) at += wave_count[w];
  at += __popcll(mask & ((1ull << (t & 63)) - 1ull));
  if (at >= a.b.m) return;   // (cannot happen: m is the sum of the counts; a store never leaves the buffers all the same)
  a.b.active[at] = p;
  ((V4*)a.b.q_points)[at] = ((const V4*)a.b.pos)[p];
  ((V4*)a.b.q_vel)[at] = ((const V4*)a.b.vel)[p];
  ((V4*)a.q_acc)[at] = ((const V4*)a.ap)[p];
  a.b.q_skip[at] = a.b.first + p;
}

// one component of the corrector (hermite6_args.hpp): v1, then x1 with it, and the crackle at the end of the step
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

// active row q of the list, row p of the slice: (x1, v1, c1) from its base and the two evaluations with its own h; the base moves to
// tau.  The fourth values of the state are the base's, that of c1 is a1's (0)
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) hermite6_block_correct(const Block6Args a) {
  const int q = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (q >= a.b.m) return;
  const int p = a.b.active[q];
  const Coefficients6<T> c = coefficients6_of(step_of<T>(a.b, p));
  const V4 x0 = ((const V4*)a.b.x0)[p], v0 = ((const V4*)a.b.v0)[p];
  const V4 a0 = ((const V4*)a.b.a0)[p], j0 = ((const V4*)a.b.j0)[p], s0 = ((const V4*)a.s0)[p];
  const V4 a1 = ((const V4*)a.b.a1)[q], j1 = ((const V4*)a.b.j1)[q], s1 = ((const V4*)a.s1)[q];
  V4 x1 = x0, v1 = v0, c1 = a1;
  const Corrected<T> rx = correct_one(c, x0.x, v0.x, a0.x, j0.x, s0.x, a1.x, j1.x, s1.x);
  const Corrected<T> ry = correct_one(c, x0.y, v0.y, a0.y, j0.y, s0.y, a1.y, j1.y, s1.y);
  const Corrected<T> rz = correct_one(c, x0.z, v0.z, a0.z, j0.z, s0.z, a1.z, j1.z, s1.z);
  x1.x = rx.x1; x1.y = ry.x1; x1.z = rz.x1;
  v1.x = rx.v1; v1.y = ry.v1; v1.z = rz.v1;
  c1.x = rx.c1; c1.y = ry.c1; c1.z = rz.c1;
  ((V4*)a.b.x0)[p] = x1;
  ((V4*)a.b.v0)[p] = v1;
  ((V4*)a.b.a0)[p] = a1;
  ((V4*)a.b.j0)[p] = j1;
  ((V4*)a.s0)[p] = s1;
  ((V4*)a.c0)[p] = c1;
  ((V4*)a.b.pos)[p] = x1;
  ((V4*)a.b.vel)[p] = v1;
  a.b.t0[p] = a.b.tau;
  a.b.level[p] = next_level(a.b.level[p], wanted_level(a1, j1, a.b.eta2, a.b.lim, a.b.levels), a.b.tau, a.b.levels);
}

inline dim3 tiles_of(int n) { return dim3((n + kLanes - 1) / kLanes); }

}  // namespace h6b
}  // namespace

namespace nbl {

NBH6B_HIDDEN int launch_hermite6_block_init_kernel(int fp64, hipStream_t st, const nbh6b::Block6Args& a) {
  using namespace h6b;
  if (bad_block6_rows(a)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite6_block_init<d4>), h6b::tiles_of(a.b.rows), dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((hermite6_block_init<f4>), h6b::tiles_of(a.b.rows), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBH6B_HIDDEN int launch_hermite6_block_predict_kernel(int fp64, hipStream_t st, const nbh6b::Block6Args& a) {
  using namespace h6b;
  if (bad_block6_predict(a)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite6_block_predict<double, d4>), h6b::tiles_of(a.b.rows), dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((hermite6_block_predict<float, f4>), h6b::tiles_of(a.b.rows), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBH6B_HIDDEN int launch_hermite6_block_compact_kernel(int fp64, hipStream_t st, const nbh6b::Block6Args& a) {
  using namespace h6b;
  if (bad_block6_compact(a)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite6_block_compact<d4>), h6b::tiles_of(a.b.rows), dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((hermite6_block_compact<f4>), h6b::tiles_of(a.b.rows), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBH6B_HIDDEN int launch_hermite6_block_correct_kernel(int fp64, hipStream_t st, const nbh6b::Block6Args& a) {
  using namespace h6b;
  if (bad_block6_correct(a)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((hermite6_block_correct<double, d4>), h6b::tiles_of(a.b.m), dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((hermite6_block_correct<float, f4>), h6b::tiles_of(a.b.m), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
