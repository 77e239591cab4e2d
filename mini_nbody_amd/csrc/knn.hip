// knn.hip — the k-nearest-neighbour pass's device code: per query the first k of the N bodies on the device in ascending (d2, j) order
// (knn_args.hpp states the rule, include/nbody.h the definition) and the combine of a split launch.  Compiles on its own; device.hip
// puts it into the library's one code object after neighbors.hip.  Reads diag_pass.hpp and nbody_args.hpp (f4, d4, NB_CONST) and
// nothing else of the force path.  d2 is the neighbour pass's: diag_pass.hpp's plain_d2, the plain squared distance; the file is
// compiled with contraction off.  No atomics, no LDS.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "knn_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbq;
using namespace nbd;

#define NBQ_HIDDEN __attribute__((visibility("hidden")))

static_assert(kKnMax == NBODY_KNN_MAX, "the header's limit is the largest list capacity");

namespace {

// What a lane carries: K (d2, idx) pairs in registers, ascending.  K is a compile-time capacity and every element index below is a
// constant after unrolling: an array indexed at run time would go to scratch memory.  The k entries of the query are the LAST k slots;
// the K - k slots before them hold (-inf, -1), which every candidate goes behind and which therefore never move.  So d[K - 1] is the
// query's k-th entry whatever k is, and a list of k entries costs k-entry traffic, not K.
template <typename T, int K>
struct KList {
  T d[K];
  int i[K];
  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      d[s] = s < K - k ? -inf_of<T>() : inf_of<T>();
      i[s] = -1;
    }
  }
  __device__ __forceinline__ T kth() const { return d[K - 1]; }
  // THE statement of record: the candidate goes behind every entry with d2 <= its own (strict <), the last entry is dropped.  From
  // the last slot down, slot s takes its left neighbour where the candidate is below that neighbour, the candidate where it is below
  // slot s only, and stays otherwise: one compare and four selects per slot.  A lane whose d2 is not below kth() — a NaN, a +inf, or
  // simply too far — changes nothing.
  __device__ __forceinline__ void insert(T d2, int j) {
    bool below = d2 < d[K - 1];
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
      const bool below_left = d2 < d[s - 1];
      d[s] = below_left ? d[s - 1] : (below ? d2 : d[s]);
      i[s] = below_left ? i[s - 1] : (below ? j : i[s]);
      below = below_left;
    }
    d[0] = below ? d2 : d[0];
    i[0] = below ? j : i[0];
  }
};

// The first walk over one aligned window of 64 sources [j, j + 64), as the neighbour pass's window64: the running minimum alone, from
// the lane's k-th entry (one v_min per pair, no index, no list).
template <bool CMP, typename T, typename V4>
__device__ __forceinline__ T knn_window_min(const NB_CONST V4* src, const V4 me, int j, int sk, T kth) {
  T wmin = kth;
#pragma unroll 8
  for (int k = 0; k < 64; ++k) wmin = min_of(wmin, plain_d2<CMP, T, V4>(src[j + k], me, j + k, sk));
  return wmin;
}

// One query per lane, kLanes queries per workgroup; workgroup (x, y) walks the blocks of chunk y for the queries of x.  Sources
// arrive with wave-uniform scalar loads (address space 4, as neighbors_kernel).  Lanes beyond m stay in the wave-uniform loops clamped
// to the last query and store nothing.  SKIP: the rows form (a.points == null: query p is source a.first + p and leaves itself out)
// and the points form with a skip array; only the aligned 64-source windows that overlap [lowest, highest] excluded index of the
// wave's 64 queries compare j with it.
template <typename T, typename V4, bool SKIP, int K>
__global__ void __launch_bounds__(kLanes) knn_kernel(KnnArgs a) {
  const auto [p, live, pc] = lane_of(a.m);
  const auto [me, sk, wlo, whi, src, s0, s1] = query_of<V4, SKIP>(a, pc);
  const int k = a.k;
  KList<T, K> c;
  c.init(k);
  // Per window: the first walk; then, only if in some lane of the wave the window's minimum is below the lane's k-th entry, the window
  // again in ascending order with the insertion — per source only if some lane inserts (wave-uniform branches).  A lane whose minimum
  // is not below its k-th entry inserts nowhere in the window: the k-th entry only falls.  The tail (N not a multiple of 64) takes the
  // second walk alone.  The second walk is the one place the insertion chain is compiled; with SKIP it always compares j with sk.
  for (int j = s0; j < s1; j += 64) {
    const int cnt = min(64, s1 - j);
    bool walk = true;
    if (cnt == 64) {
      const T kth = c.kth();
      const T wmin = !SKIP || j + 63 < wlo || j > whi ? knn_window_min<false, T, V4>(src, me, j, sk, kth)
                                                       : knn_window_min<true, T, V4>(src, me, j, sk, kth);
      walk = __ballot(wmin < kth) != 0;
    }
    if (!walk) continue;
#pragma unroll 1
    for (int q = 0; q < cnt; ++q) {
      const T d2 = plain_d2<SKIP, T, V4>(src[j + q], me, j + q, sk);
      if (__ballot(d2 < c.kth()) != 0) c.insert(d2, j + q);
    }
  }
  if (!live) return;
  // entry r is slot K - k + r
  if (a.scratch) {
    T* sd = (T*)knn_scratch_d2(a);
    int* si = knn_scratch_idx(a, sizeof(T));
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const int r = s - (K - k);
      if (r < 0) continue;
      const size_t w = knn_scratch_at(a, (int)blockIdx.y, r, p);
      sd[w] = c.d[s];
      si[w] = c.i[s];
    }
  } else {
    const size_t w0 = (size_t)p * (size_t)k;
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const int r = s - (K - k);
      if (r < 0) continue;
      if (a.idx) a.idx[w0 + (size_t)r] = c.i[s];
      if (a.d2) ((T*)a.d2)[w0 + (size_t)r] = c.d[s];
    }
  }
}

// the chunks of a split launch in ascending order, each chunk's entries in ascending order, through the same insertion; one query per
// lane (a wave reads 64 consecutive values).  A chunk's padding (+inf, -1) is below nothing and is never inserted.
template <typename T, int K>
__global__ void __launch_bounds__(kLanes) knn_combine(KnnArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (p >= a.m) return;
  const T* sd = (const T*)knn_scratch_d2(a);
  const int* si = knn_scratch_idx(a, sizeof(T));
  const int k = a.k;
  KList<T, K> c;
  c.init(k);
  for (int y = 0; y < a.chunks; ++y) {
#pragma unroll 1
    for (int r = 0; r < k; ++r) {
      const size_t w = knn_scratch_at(a, y, r, p);
      const T d2 = sd[w];
      if (d2 < c.kth()) c.insert(d2, si[w]);
    }
  }
  const size_t w0 = (size_t)p * (size_t)k;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const int r = s - (K - k);
    if (r < 0) continue;
    if (a.idx) a.idx[w0 + (size_t)r] = c.i[s];
    if (a.d2) ((T*)a.d2)[w0 + (size_t)r] = c.d[s];
  }
}

template <typename T, typename V4, int K>
void launch_knn_one(hipStream_t st, const KnnArgs& a) {
  const dim3 grid((a.m + kLanes - 1) / kLanes, a.chunks), block(kLanes);
  if (!a.points || a.skip) hipLaunchKernelGGL((knn_kernel<T, V4, true, K>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((knn_kernel<T, V4, false, K>), grid, block, 0, st, a);
}

template <typename T, typename V4>
void launch_knn_of(hipStream_t st, const KnnArgs& a) {
  switch (knn_capacity(a.k)) {
    case 4: launch_knn_one<T, V4, 4>(st, a); break;
    case 8: launch_knn_one<T, V4, 8>(st, a); break;
    case 16: launch_knn_one<T, V4, 16>(st, a); break;
    default: launch_knn_one<T, V4, 32>(st, a); break;
  }
}

template <typename T>
void launch_knn_combine_of(hipStream_t st, const KnnArgs& a) {
  const dim3 grid((a.m + kLanes - 1) / kLanes), block(kLanes);
  switch (knn_capacity(a.k)) {
    case 4: hipLaunchKernelGGL((knn_combine<T, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((knn_combine<T, 8>), grid, block, 0, st, a); break;
    case 16: hipLaunchKernelGGL((knn_combine<T, 16>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((knn_combine<T, 32>), grid, block, 0, st, a); break;
  }
}

}  // namespace

namespace nbl {

NBQ_HIDDEN int launch_knn_kernel(int fp64, hipStream_t st, const KnnArgs& a) {
  if (bad_knn_launch(a)) return (int)hipErrorInvalidValue;
  if (fp64) launch_knn_of<double, d4>(st, a);
  else launch_knn_of<float, f4>(st, a);
  return (int)hipGetLastError();
}

NBQ_HIDDEN int launch_knn_combine_kernel(int fp64, hipStream_t st, const KnnArgs& a) {
  if (bad_knn_combine(a)) return (int)hipErrorInvalidValue;
  if (fp64) launch_knn_combine_of<double>(st, a);
  else launch_knn_combine_of<float>(st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
