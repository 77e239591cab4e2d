// hist.hip — the radial-count pass's device code: per query the number of the N bodies on the device in each of n_bins shells of
// squared distance (hist_args.hpp states the rule, include/nbody.h the definition), the combine of a split launch and the reduction of
// a device's rows to the 64-bit sums of the pair histogram.  Compiles on its own; device.hip puts it into the library's one code object
// after fof.hip.  Reads diag_pass.hpp and nbody_args.hpp (f4, d4, NB_CONST) and nothing else of the force path.  d2 is the neighbour
// pass's: diag_pass.hpp's plain_d2, the plain squared distance; the file is compiled with contraction off.  The kernel and the
// combine use no atomics and no LDS; the reduction adds integers with LDS and 64-bit integer atomics.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "hist_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbh;
using namespace nbd;

#define NBH_HIDDEN __attribute__((visibility("hidden")))

static_assert(kHistMaxBins == NBODY_HIST_MAX_BINS, "the header's limit is the largest capacity");

namespace {

// What a lane carries: the C + 1 cumulative counters c[s] = #{ j : d2_j < e[s] } in registers, beside the wave-uniform edges e[s].
// C is a compile-time capacity and every element index below is a constant after unrolling: an array indexed at run time would go to
// scratch memory.  The n_bins + 1 edges of the query are the LAST slots; the C - n_bins slots before them hold -inf, which nothing is
// below, so their counters stay 0.  They are compared all the same: a query costs its capacity's C + 1 compares per pair, not its
// own n_bins + 1 — at most 1.83 x its own from three bins up (17 bins: 33 against 18), but 5 against 2 (2.5 x) at one bin and 5
// against 3 at two, there being no capacity below 4.
// Where the edges live: they are read from the kernel argument block at constant offsets, wave-uniform.  fp32 up to C = 16: C + 1
// SGPRs.  fp64 at C = 32 would need 66 SGPRs beside the loop's own and the compares' lane masks, past the 102-SGPR budget, and fp32 at
// C = 32 came out with spilled SGPRs (and 20 bytes of scratch in one form) for the same reason; so the fp64 edges at every capacity
// and the fp32 edges at C = 32 are moved to VGPRs once before the loop (vgpr_of): C + 1 or 2 (C + 1) VGPRs, inside a 256-lane
// workgroup's 256 at every capacity, and the compare reads them at no extra cost.  With that and the scheduling barriers in count()
// no instantiation spills a register of either kind or has scratch (DESIGN.md §3.12 has the table).
template <typename T, int C>
struct Cum {
  T e[C + 1];
  int c[C + 1];
  __device__ __forceinline__ void init(const HistArgs& a) {
    const T* slot = (const T*)a.edges + (kHistSlots - (C + 1));
#pragma unroll
    for (int s = 0; s <= C; ++s) {
      e[s] = kEdgesInVgprs ? vgpr_of(slot[s]) : slot[s];
      c[s] = 0;
    }
  }
  static constexpr bool kEdgesInVgprs = sizeof(T) == 8 || C == 32;
  __device__ __forceinline__ static float vgpr_of(float v) {
    asm volatile("" : "+v"(v));
    return v;
  }
  __device__ __forceinline__ static double vgpr_of(double v) {
    asm volatile("" : "+v"(v));
    return v;
  }
  __device__ __forceinline__ T last() const { return e[C]; }
  // THE statement of record: one compare and one add-with-carry per edge.  A NaN d2 (the excluded body's, or one that the positions
  // made) and a d2 that is not below the last edge change nothing.
  __device__ __forceinline__ void count(T d2) {
#pragma unroll
    for (int s = 0; s <= C; ++s) {
      c[s] += d2 < e[s] ? 1 : 0;
      // every compare leaves a 64-bit lane mask in SGPRs: keep the scheduler from gathering more than eight of them ahead of their adds
      if (C > 8 && s % 8 == 7) __builtin_amdgcn_sched_barrier(0);
    }
  }
};

// one aligned window of 64 sources [j, j + 64) with the counters
template <bool CMP, typename T, typename V4, int C>
__device__ __forceinline__ void count_window(const NB_CONST V4* src, const V4 me, int j, int sk, Cum<T, C>& c) {
#pragma unroll 2
  for (int k = 0; k < 64; ++k) c.count(plain_d2<CMP, T, V4>(src[j + k], me, j + k, sk));
}
// and its first walk in the gated form, as the neighbour pass's window64: the running minimum alone (one v_min per pair)
template <bool CMP, typename T, typename V4>
__device__ __forceinline__ T window_min(const NB_CONST V4* src, const V4 me, int j, int sk) {
  T wmin = inf_of<T>();
#pragma unroll 8
  for (int k = 0; k < 64; ++k) wmin = min_of(wmin, plain_d2<CMP, T, V4>(src[j + k], me, j + k, sk));
  return wmin;
}

// One query per lane, kLanes queries per workgroup; workgroup (x, y) walks the blocks of chunk y for the queries of x.  Sources
// arrive with wave-uniform scalar loads (address space 4, as neighbors_kernel).  Lanes beyond m stay in the wave-uniform loops clamped
// to the last query and store nothing.  SKIP: the rows form (a.points == null: query p is source a.first + p and leaves itself out)
// and the points form with a skip array; only the aligned 64-source windows that overlap [lowest, highest] excluded index of the
// wave's 64 queries compare j with it (a wave-uniform branch).  LOOP == kHistLoopGated: a window is walked with the counters only if in
// some lane of the wave its minimum is below the last edge — no d2 of a window that is not walked is below any edge, the edges being
// non-decreasing.  The tail (N not a multiple of 64) is counted pair by pair.
template <typename T, typename V4, bool SKIP, int C, int LOOP>
__global__ void __launch_bounds__(kLanes) hist_kernel(HistArgs a) {
  const auto [p, live, pc] = lane_of(a.m);
  const auto [me, sk, wlo, whi, src, s0, s1] = query_of<V4, SKIP>(a, pc);
  Cum<T, C> c;
  c.init(a);
  int j = s0;
  for (; j + 64 <= s1; j += 64) {
    const bool plain = !SKIP || j + 63 < wlo || j > whi;
    if constexpr (LOOP == kHistLoopGated) {
      const T wmin = plain ? window_min<false, T, V4>(src, me, j, sk) : window_min<true, T, V4>(src, me, j, sk);
      if (__ballot(wmin < c.last()) == 0) continue;   // wave-uniform
    }
    if (plain) count_window<false, T, V4, C>(src, me, j, sk, c);
    else count_window<true, T, V4, C>(src, me, j, sk, c);
  }
  for (; j < s1; ++j) c.count(plain_d2<SKIP, T, V4>(src[j], me, j, sk));
  if (!live) return;
  // bin b is slots C - n_bins + b and the one after it
  const int nb = a.n_bins;
#pragma unroll
  for (int s = 0; s < C; ++s) {
    const int b = s - (C - nb);
    if (b < 0) continue;
    const int v = c.c[s + 1] - c.c[s];
    if (a.scratch) a.scratch[hist_scratch_at(a, (int)blockIdx.y, b, p)] = v;
    else a.counts[(size_t)p * (size_t)nb + (size_t)b] = v;
  }
}

// the chunks of a split launch added per (query, bin): one query per lane (a wave reads 64 consecutive values), one bin per
// blockIdx.y — a lane that took all n_bins bins of its query read chunks x n_bins values one after the other, and at m = 256 over 512
// chunks of 32 bins that was most of the call (profiles/r10_hist_rate.txt)
__global__ void __launch_bounds__(kLanes) hist_combine(HistArgs a) {
  const int p = (int)blockIdx.x * kLanes + (int)threadIdx.x, b = (int)blockIdx.y;
  if (p >= a.m) return;
  int v = 0;
  for (int y = 0; y < a.chunks; ++y) v += a.scratch[hist_scratch_at(a, y, b, p)];
  a.counts[(size_t)p * (size_t)a.n_bins + (size_t)b] = v;
}

// A batch of rows' counts into the device's 64-bit sums.  Lane t takes bin t % 32 of rows t / 32, t / 32 + 8 G, ... (G workgroups of
// 8 rows at a time), the 8 partial sums of a bin meet in LDS and one lane per bin adds them to sums[b] with a 64-bit integer atomic.
// Integer sums: the same values in every order.
constexpr int kReduceRows = kLanes / kHistMaxBins;
__global__ void __launch_bounds__(kLanes) hist_reduce(const int* counts, int rows, int n_bins, unsigned long long* sums) {
  __shared__ unsigned long long part[kLanes];
  const int t = (int)threadIdx.x, b = t % kHistMaxBins, rg = t / kHistMaxBins;
  unsigned long long acc = 0;
  if (b < n_bins)
    for (long long r = (long long)blockIdx.x * kReduceRows + rg; r < rows; r += (long long)gridDim.x * kReduceRows)
      acc += (unsigned long long)counts[(size_t)r * (size_t)n_bins + (size_t)b];
  part[t] = acc;
  __syncthreads();
  if (rg != 0 || b >= n_bins) return;
  for (int q = 1; q < kReduceRows; ++q) acc += part[q * kHistMaxBins + b];
  if (acc) atomicAdd(&sums[b], acc);
}

template <typename T, typename V4, int C, int LOOP>
void launch_hist_one(hipStream_t st, const HistArgs& a) {
  const dim3 grid((a.m + kLanes - 1) / kLanes, a.chunks), block(kLanes);
  if (!a.points || a.skip) hipLaunchKernelGGL((hist_kernel<T, V4, true, C, LOOP>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((hist_kernel<T, V4, false, C, LOOP>), grid, block, 0, st, a);
}

template <typename T, typename V4, int LOOP>
void launch_hist_of(hipStream_t st, const HistArgs& a) {
  switch (hist_capacity(a.n_bins)) {
    case 4: launch_hist_one<T, V4, 4, LOOP>(st, a); break;
    case 8: launch_hist_one<T, V4, 8, LOOP>(st, a); break;
    case 16: launch_hist_one<T, V4, 16, LOOP>(st, a); break;
    default: launch_hist_one<T, V4, 32, LOOP>(st, a); break;
  }
}

}  // namespace

namespace nbl {

NBH_HIDDEN int launch_hist_kernel(int fp64, int loop, hipStream_t st, const HistArgs& a) {
  if (bad_hist_launch(a)) return (int)hipErrorInvalidValue;
  if (fp64) {
    if (loop == kHistLoopGated) launch_hist_of<double, d4, kHistLoopGated>(st, a);
    else launch_hist_of<double, d4, kHistLoopScan>(st, a);
  } else {
    if (loop == kHistLoopGated) launch_hist_of<float, f4, kHistLoopGated>(st, a);
    else launch_hist_of<float, f4, kHistLoopScan>(st, a);
  }
  return (int)hipGetLastError();
}

NBH_HIDDEN int launch_hist_combine_kernel(hipStream_t st, const HistArgs& a) {
  if (bad_hist_combine(a)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(hist_combine, dim3((a.m + kLanes - 1) / kLanes, a.n_bins), dim3(kLanes), 0, st, a);
  return (int)hipGetLastError();
}

NBH_HIDDEN int launch_hist_reduce_kernel(hipStream_t st, const int* counts, int rows, int n_bins, unsigned long long* sums) {
  if (bad_hist_reduce(counts, rows, n_bins, sums)) return (int)hipErrorInvalidValue;
  if (rows == 0) return (int)hipSuccess;
  const int groups = std::min((rows + kReduceRows - 1) / kReduceRows, 1024);
  hipLaunchKernelGGL(hist_reduce, dim3(groups), dim3(kLanes), 0, st, counts, rows, n_bins, sums);
  return (int)hipGetLastError();
}

}  // namespace nbl
