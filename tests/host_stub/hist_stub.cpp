// hist_stub.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py, case `hist`): a host-only stand-in for the launch functions of hist.hip,
// linked beside hip_stub.cpp so that hist.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.  hip_stub.cpp's streams
// are synchronous and the pass is never captured, so all three functions execute at launch.
// The stand-in pushes values a test can predict through the REAL HistArgs — the right-aligned edge slots, chunk bounds, the chunks'
// scratch layout [chunk][bin][m], the combine's sums, pointers the host offset per local and per batch, the [m][n_bins] outputs, the
// rows form's first, the reduction's 64-bit sums — so ASan sees every offset the host computed.  Per query p (stub_common.hpp: the word
// q and the excluded body sk) every block b offers the ONE body of stub_rule.hpp (j_b, d2_b; none if j_b == sk), as neighbors_stub.cpp's
// and knn_stub.cpp's, counted by the cumulative rule, c_s += d2_b < edge_s, bin b = c_(b+1) - c_b.  It says nothing about the kernels'
// arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include "../../mini_nbody_amd/csrc/hist_args.hpp"
#include "stub_common.hpp"

namespace {

using namespace nbh;

// the counts of blocks [b0, b1) for query p
template <typename T>
void chunk(const HistArgs& a, int p, int b0, int b1, int* bins) {
  const auto [q, sk] = stub::query_of<T>(a, p);
  const T* edge = (const T*)a.edges + (kHistSlots - (a.n_bins + 1));   // the query's edges are the last n_bins + 1 slots
  int cum[kHistSlots] = {0};
  for (int b = b0; b < b1; ++b) {
    const int j = stub::candidate(a.n_src, q.w, b).j;
    if (j == sk) continue;
    const T d2 = stub::absdiff(((const stub::W4<T>*)a.src)[j].x, q.x);
    for (int s = 0; s <= a.n_bins; ++s) cum[s] += d2 < edge[s];
  }
  for (int s = 0; s < a.n_bins; ++s) bins[s] = cum[s + 1] - cum[s];
}

template <typename T>
void hist(const HistArgs& a) {
  const T* lead = (const T*)a.edges;
  for (int s = 0; s < kHistSlots - (a.n_bins + 1); ++s)
    if (!(lead[s] < 0 && lead[s] * 2 == lead[s])) abort();   // the slots before the query's edges hold -inf
  stub::for_each_chunk(a, [&](int p, int y, int b0, int b1) {
    int bins[kHistMaxBins];
    chunk<T>(a, p, b0, b1, bins);
    for (int b = 0; b < a.n_bins; ++b) {
      if (a.scratch) a.scratch[hist_scratch_at(a, y, b, p)] = bins[b];
      else a.counts[(size_t)p * (size_t)a.n_bins + (size_t)b] = bins[b];
    }
  });
}

}  // namespace

// combine launches so far: one per batch of a split launch, none when the sources are not split; reduce launches: one per batch of rows
STUB_COUNTER(hist_stub_combines)
STUB_COUNTER(hist_stub_reduces)

namespace nbl {
int launch_hist_kernel(int fp64, int loop, hipStream_t, const nbh::HistArgs& a) {
  if (nbh::bad_hist_launch(a)) return (int)hipErrorInvalidValue;
  if (loop != nbh::kHistLoopScan && loop != nbh::kHistLoopGated) return (int)hipErrorInvalidValue;   // the stub's own: the host passes no other
  if (fp64) hist<double>(a); else hist<float>(a);
  return 0;
}
int launch_hist_combine_kernel(hipStream_t, const nbh::HistArgs& a) {
  if (nbh::bad_hist_combine(a)) return (int)hipErrorInvalidValue;
  g_hist_stub_combines.fetch_add(1);
  for (int p = 0; p < a.m; ++p)
    for (int b = 0; b < a.n_bins; ++b) {
      int v = 0;
      for (int y = 0; y < a.chunks; ++y) v += a.scratch[nbh::hist_scratch_at(a, y, b, p)];
      a.counts[(size_t)p * (size_t)a.n_bins + (size_t)b] = v;
    }
  return 0;
}
int launch_hist_reduce_kernel(hipStream_t, const int* counts, int rows, int n_bins, unsigned long long* sums) {
  if (nbh::bad_hist_reduce(counts, rows, n_bins, sums)) return (int)hipErrorInvalidValue;
  g_hist_stub_reduces.fetch_add(1);
  for (int r = 0; r < rows; ++r)
    for (int b = 0; b < n_bins; ++b) sums[b] += (unsigned long long)counts[(size_t)r * (size_t)n_bins + (size_t)b];
  return 0;
}
}  // namespace nbl
