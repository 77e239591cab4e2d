// neighbors.hip — the neighbour pass's device code: per query the nearest of the N bodies on the device, its squared distance and the
// number of bodies within a radius (neighbors_args.hpp states the rule, include/nbody.h the definitions), the combine of a split launch
// and the fixed-order reduction of a device's rows to its closest pair.  Compiles on its own; device.hip puts it into the library's
// one code object after point_sums.hip.  Reads nbody_args.hpp (f4, d4, NB_CONST) and nothing else of the force path.  d2 is
// diag_pass.hpp's plain_d2, the plain squared distance; the file is compiled with contraction off.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "neighbors_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbn;
using namespace nbd;

#define NBN_HIDDEN __attribute__((visibility("hidden")))

namespace {

// what a lane carries: the ascending scan's state
template <typename T>
struct Near { T best; int idx, cnt; };

// the statement of record: one pair of the ascending scan that replaces on strict < (compare, two selects; compare and add for the count)
template <bool CMP, bool COUNT, typename T, typename V4>
__device__ __forceinline__ void scan_pair(const V4 p, const V4 me, int j, int sk, T r2, Near<T>& c) {
  const T d2 = plain_d2<CMP, T, V4>(p, me, j, sk);
  const bool less = d2 < c.best;
  c.best = less ? d2 : c.best;
  c.idx = less ? j : c.idx;
  if (COUNT) c.cnt += d2 <= r2 ? 1 : 0;
}

// One aligned window of 64 sources [j, j + 64) without an index in the loop: the running minimum alone (one v_min per pair), then,
// only if a lane of the wave improved, the window again from its last source down to its first, so that the lowest j with
// d2 == the new minimum is the one that stays — what the ascending scan with strict < arrives at: it replaces at the first source that
// reaches the window's minimum and at none of the later equal ones.  A lane that did not improve keeps its index.
template <bool CMP, bool COUNT, typename T, typename V4>
__device__ __forceinline__ void window64(const NB_CONST V4* src, const V4 me, int j, int sk, T r2, Near<T>& c) {
  T wmin = c.best;
#pragma unroll 8
  for (int k = 0; k < 64; ++k) {
    const T d2 = plain_d2<CMP, T, V4>(src[j + k], me, j + k, sk);
    wmin = min_of(wmin, d2);
    if (COUNT) c.cnt += d2 <= r2 ? 1 : 0;
  }
  const bool improved = wmin < c.best;
  if (__ballot(improved) != 0) {   // wave-uniform
    int widx = -1;
#pragma unroll 8
    for (int k = 63; k >= 0; --k) {
      const T d2 = plain_d2<CMP, T, V4>(src[j + k], me, j + k, sk);
      widx = d2 == wmin ? j + k : widx;
    }
    c.idx = improved ? widx : c.idx;
    c.best = wmin;
  }
}

// One query per lane, kLanes queries per workgroup; workgroup (x, y) walks the blocks of chunk y for the queries of x.  Sources
// arrive with wave-uniform scalar loads (address space 4, as block_sums_kernel).  Lanes beyond m stay in the wave-uniform loops clamped to
// the last query and store nothing.  SKIP: the rows form (a.points == null: query p is source a.first + p and leaves itself out) and
// the points form with a skip array; only the aligned 64-source windows that overlap [lowest, highest] excluded index of the wave's
// 64 queries compare j with it (a wave-uniform branch) — in the rows form the one or two windows that hold the wave's own rows.
template <typename T, typename V4, bool SKIP, bool COUNT, int LOOP>
__global__ void __launch_bounds__(kLanes) neighbors_kernel(NeighborsArgs a) {
  const auto [p, live, pc] = lane_of(a.m);
  const auto [me, sk, wlo, whi, src, s0, s1] = query_of<V4, SKIP>(a, pc);
  const T r2 = (T)a.r2;
  Near<T> c = {inf_of<T>(), -1, 0};
  int j = s0;
  for (; j + 64 <= s1; j += 64) {
    if (!SKIP || j + 63 < wlo || j > whi) {
      if constexpr (LOOP == kNbLoopWindow) {
        window64<false, COUNT, T, V4>(src, me, j, sk, r2, c);
      } else {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) scan_pair<false, COUNT, T, V4>(src[j + k], me, j + k, sk, r2, c);
      }
    } else {
      if constexpr (LOOP == kNbLoopWindow) {
        window64<true, COUNT, T, V4>(src, me, j, sk, r2, c);
      } else {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) scan_pair<true, COUNT, T, V4>(src[j + k], me, j + k, sk, r2, c);
      }
    }
  }
  for (; j < s1; ++j) scan_pair<SKIP, COUNT, T, V4>(src[j], me, j, sk, r2, c);   // the tail (N not a multiple of 64)
  if (!live) return;
  if (a.scratch) {
    const size_t w = (size_t)blockIdx.y * (size_t)a.m + (size_t)p;
    ((T*)scratch_d2(a))[w] = c.best;
    scratch_idx(a, sizeof(T))[w] = c.idx;
    if (COUNT) scratch_count(a, sizeof(T))[w] = c.cnt;
  } else {
    if (a.idx) a.idx[p] = c.idx;
    if (a.d2) ((T*)a.d2)[p] = c.best;
    if (COUNT) a.count[p] = c.cnt;
  }
}

// the chunks of a split launch in ascending order: strict <, counts added; one query per lane (a wave reads 64 consecutive values)
template <typename T>
__global__ void __launch_bounds__(kLanes) neighbors_combine(NeighborsArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.m) return;
  const T* sd = (const T*)scratch_d2(a);
  const int* si = scratch_idx(a, sizeof(T));
  const int* sn = scratch_count(a, sizeof(T));
  Near<T> c = {inf_of<T>(), -1, 0};
  for (int y = 0; y < a.chunks; ++y) {
    const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
    const T d2 = sd[w];
    if (d2 < c.best) { c.best = d2; c.idx = si[w]; }
    if (a.count) c.cnt += sn[w];
  }
  if (a.idx) a.idx[p] = c.idx;
  if (a.d2) ((T*)a.d2)[p] = c.best;
  if (a.count) a.count[p] = c.cnt;
}

// the closest pair of a device's rows: lane t takes rows t, t + 256, ... ascending with strict <, lane 0 then the 256 lanes' bests by
// (d2, row).  One workgroup, no atomics.  The lowest row that reaches the smallest d2 is the pair's i and its neighbour the pair's j.
template <typename T>
__global__ void __launch_bounds__(kLanes) neighbors_best(const T* d2, const int* idx, int rows, int first, BestPair* out) {
  __shared__ double sd[kLanes];
  __shared__ int sr[kLanes];
  const int t = (int)threadIdx.x;
  T best = inf_of<T>();
  int row = -1;
  for (int r = t; r < rows; r += kLanes) {
    const T v = d2[r];
    if (v < best) { best = v; row = r; }
  }
  sd[t] = (double)best;
  sr[t] = row;
  __syncthreads();
  if (t != 0) return;
  double b = (double)inf_of<T>();
  int br = -1;
  for (int q = 0; q < kLanes; ++q) {
    if (sr[q] >= 0 && (sd[q] < b || (sd[q] == b && sr[q] < br))) { b = sd[q]; br = sr[q]; }
  }
  out->d2 = b;
  out->i = br < 0 ? -1 : first + br;
  out->j = br < 0 ? -1 : idx[br];
}

template <typename T, typename V4, int LOOP>
void launch_neighbors_one(hipStream_t st, const NeighborsArgs& a) {
  const dim3 grid((a.m + kLanes - 1) / kLanes, a.chunks), block(kLanes);
  const bool skip = !a.points || a.skip;
  if (skip && a.count) hipLaunchKernelGGL((neighbors_kernel<T, V4, true, true, LOOP>), grid, block, 0, st, a);
  else if (skip) hipLaunchKernelGGL((neighbors_kernel<T, V4, true, false, LOOP>), grid, block, 0, st, a);
  else if (a.count) hipLaunchKernelGGL((neighbors_kernel<T, V4, false, true, LOOP>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((neighbors_kernel<T, V4, false, false, LOOP>), grid, block, 0, st, a);
}

}  // namespace

namespace nbl {

NBN_HIDDEN int launch_neighbors_kernel(int fp64, int loop, hipStream_t st, const NeighborsArgs& a) {
  if (bad_source_split(a, !a.points)) return (int)hipErrorInvalidValue;
  if (fp64) {
    if (loop == kNbLoopScan) launch_neighbors_one<double, d4, kNbLoopScan>(st, a);
    else launch_neighbors_one<double, d4, kNbLoopWindow>(st, a);
  } else {
    if (loop == kNbLoopScan) launch_neighbors_one<float, f4, kNbLoopScan>(st, a);
    else launch_neighbors_one<float, f4, kNbLoopWindow>(st, a);
  }
  return (int)hipGetLastError();
}

NBN_HIDDEN int launch_neighbors_combine_kernel(int fp64, hipStream_t st, const NeighborsArgs& a) {
  if (bad_combine(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes);
  if (fp64) hipLaunchKernelGGL((neighbors_combine<double>), grid, dim3(kLanes), 0, st, a);
  else hipLaunchKernelGGL((neighbors_combine<float>), grid, dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBN_HIDDEN int launch_neighbors_best_kernel(int fp64, hipStream_t st, const void* d2, const int* idx, int rows, int first, BestPair* out) {
  if (bad_row_reduce(rows, out, d2 && idx)) return (int)hipErrorInvalidValue;
  if (fp64) hipLaunchKernelGGL((neighbors_best<double>), dim3(1), dim3(kLanes), 0, st, (const double*)d2, idx, rows, first, out);
  else hipLaunchKernelGGL((neighbors_best<float>), dim3(1), dim3(kLanes), 0, st, (const float*)d2, idx, rows, first, out);
  return (int)hipGetLastError();
}

}  // namespace nbl
