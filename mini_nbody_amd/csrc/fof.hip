// fof.hip — the friends-of-friends link pass's device code: per row the lowest foreign label among the bodies within the linking length
// (fof_args.hpp states the rule, include/nbody.h the definitions) and the combine of a split launch.  Compiles on its own; device.hip
// puts it into the library's one code object after knn.hip.  Reads nbody_args.hpp (f4, d4, NB_CONST) and nothing else of the force
// path.  d2 is the neighbour pass's: diag_pass.hpp's plain_d2, the plain squared distance; the file is compiled with contraction
// off.  No atomics, no LDS.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "fof_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbg;
using namespace nbd;

#define NBG_HIDDEN __attribute__((visibility("hidden")))

namespace {

// the statement of record: one pair of the link pass.  A NaN d2 links nothing; the row itself (and every body of its own group) drops
// out by its label, so no index is compared
template <typename T, typename V4>
__device__ __forceinline__ int link_pair(const V4 p, int lj, const V4 me, int mine, T b2, int m) {
  const T d2 = plain_d2<T, V4>(p, me);
  return (d2 <= b2 && lj != mine) ? min(m, lj) : m;
}

// One aligned window of 64 sources [j, j + 64), neighbors.hip's window64 generalised: first only "did any source come within b2" — the
// running minimum of d2 (one v_min per pair, no label loaded) — then, only if a lane of the wave had one, the window again with the
// labels beside the positions.  At small linking lengths almost no window is walked twice.
template <typename T, typename V4>
__device__ __forceinline__ int link_window(const NB_CONST V4* src, const NB_CONST int* lab, const V4 me, int mine, int j, T b2, int m) {
  T wmin = inf_of<T>();
#pragma unroll 8
  for (int k = 0; k < 64; ++k) wmin = min_of(wmin, plain_d2<T, V4>(src[j + k], me));
  if (__ballot(wmin <= b2) != 0) {   // wave-uniform
#pragma unroll 8
    for (int k = 0; k < 64; ++k) m = link_pair<T, V4>(src[j + k], lab[j + k], me, mine, b2, m);
  }
  return m;
}

// One row per lane, kLanes rows per workgroup; workgroup (x, y) walks the blocks of chunk y for the rows of x.  Sources and their
// labels arrive with wave-uniform scalar loads (address space 4, as neighbors_kernel).  Lanes beyond m stay in the wave-uniform loops
// clamped to the last row and store nothing.  Row p is body a.rows[p] (the active rows of a later round) or a.first + p.
template <typename T, typename V4>
__global__ void __launch_bounds__(kLanes) fof_kernel(FofArgs a) {
  const auto [p, live, pc] = lane_of(a.m);
  const int i = a.rows ? a.rows[pc] : a.first + pc;
  const V4 me = ((const V4*)a.src)[i];
  const int mine = a.label[i];
  const T b2 = (T)a.b2;
  const NB_CONST V4* src = scalar_src<V4>(a.src);
  const NB_CONST int* lab = scalar_src<int>(a.label);
  const auto [s0, s1] = chunk_sources(a);
  int m = kFoNone;
  int j = s0;
  for (; j + 64 <= s1; j += 64) m = link_window<T, V4>(src, lab, me, mine, j, b2, m);
  for (; j < s1; ++j) m = link_pair<T, V4>(src[j], lab[j], me, mine, b2, m);   // the tail (N not a multiple of 64)
  if (!live) return;
  if (a.scratch) a.scratch[(size_t)blockIdx.y * (size_t)a.m + (size_t)p] = m;
  else a.out[p] = m;
}

// the minimum over the chunks of a split launch; one row per lane (a wave reads 64 consecutive values)
__global__ void __launch_bounds__(kLanes) fof_combine(FofArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.m) return;
  int m = kFoNone;
  for (int y = 0; y < a.chunks; ++y) m = min(m, a.scratch[(size_t)y * (size_t)a.m + (size_t)p]);
  a.out[p] = m;
}

}  // namespace

namespace nbl {

NBG_HIDDEN int launch_fof_kernel(int fp64, hipStream_t st, const FofArgs& a) {
  if (bad_fof_launch(a)) return (int)hipErrorInvalidValue;
  const dim3 grid((a.m + kLanes - 1) / kLanes, a.chunks), block(kLanes);
  if (fp64) hipLaunchKernelGGL((fof_kernel<double, d4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((fof_kernel<float, f4>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

NBG_HIDDEN int launch_fof_combine_kernel(hipStream_t st, const FofArgs& a) {
  if (bad_fof_combine(a)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(fof_combine, dim3((a.m + kLanes - 1) / kLanes), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
