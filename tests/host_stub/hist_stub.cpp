// hist_stub.cpp — TEST INFRASTRUCTURE (tests/test_hist_host_sanitizers.py): a host-only stand-in for the launch functions of hist.hip,
// linked beside hip_stub.cpp so that hist.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.  hip_stub.cpp's streams
// are synchronous and the pass is never captured, so all three functions execute at launch.
// The stand-in pushes values a test can predict through the REAL HistArgs — the right-aligned edge slots, chunk bounds, the chunks'
// scratch layout [chunk][bin][m], the combine's sums, pointers the host offset per local and per batch, the [m][n_bins] outputs, the
// rows form's first, the reduction's 64-bit sums — so ASan sees every offset the host computed.  Per query p (q = points[p], or in the
// rows form source first + p; sk = skip[p], -1, or in the rows form first + p) every block b of 1024 sources (len_b of them) offers ONE
// body, as neighbors_stub.cpp's and knn_stub.cpp's:
//   j_b = 1024 b + ((int)q.w + b) mod len_b      d2_b = |src[j_b].x - q.x|      (none if j_b == sk)
// counted by the cumulative rule, c_s += d2_b < edge_s, bin b = c_(b+1) - c_b; q.w, which the real kernel ignores, lets a driver steer
// the bodies.  It says nothing about the kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "../../mini_nbody_amd/csrc/hist_args.hpp"

namespace {

using namespace nbh;

template <typename T>
struct W4 { T x, y, z, w; };

// the counts of chunk y of query p
template <typename T>
void chunk(const HistArgs& a, int p, int y, int* bins) {
  typedef W4<T> V;
  const V* src = (const V*)a.src;
  const V q = a.points ? ((const V*)a.points)[p] : src[a.first + p];
  const int sk = a.points ? (a.skip ? a.skip[p] : -1) : a.first + p;
  const T* edge = (const T*)a.edges + (kHistSlots - (a.n_bins + 1));   // the query's edges are the last n_bins + 1 slots
  int cum[kHistSlots] = {0};
  const int blk1 = std::min((y + 1) * a.chunk_blocks, a.n_blocks);
  for (int b = y * a.chunk_blocks; b < blk1; ++b) {
    const int b0 = b * nbd::kSrcBlock, len = std::min(nbd::kSrcBlock, a.n_src - b0);
    const int j = b0 + ((int)q.w + b) % len;
    const T d = src[j].x - q.x, d2 = d < 0 ? -d : d;
    if (j == sk) continue;
    for (int s = 0; s <= a.n_bins; ++s) cum[s] += d2 < edge[s];
  }
  for (int s = 0; s < a.n_bins; ++s) bins[s] = cum[s + 1] - cum[s];
}

template <typename T>
void hist(const HistArgs& a) {
  const T* lead = (const T*)a.edges;
  for (int s = 0; s < kHistSlots - (a.n_bins + 1); ++s)
    if (!(lead[s] < 0 && lead[s] * 2 == lead[s])) abort();   // the slots before the query's edges hold -inf
  for (int p = 0; p < a.m; ++p)
    for (int y = 0; y < a.chunks; ++y) {
      int bins[kHistMaxBins];
      chunk<T>(a, p, y, bins);
      for (int b = 0; b < a.n_bins; ++b) {
        if (a.scratch) a.scratch[hist_scratch_at(a, y, b, p)] = bins[b];
        else a.counts[(size_t)p * (size_t)a.n_bins + (size_t)b] = bins[b];
      }
    }
}

std::atomic<long> g_combines{0}, g_reduces{0};

}  // namespace

// combine launches so far: one per batch of a split launch, none when the sources are not split; reduce launches: one per batch of rows
extern "C" long hist_stub_combines(void) { return g_combines.load(); }
extern "C" long hist_stub_reduces(void) { return g_reduces.load(); }

namespace nbl {
int launch_hist_kernel(int fp64, int loop, hipStream_t, const nbh::HistArgs& a) {
  if (nbd::bad_source_split(a, !a.points) || a.n_bins < 1 || a.n_bins > nbh::kHistMaxBins) return (int)hipErrorInvalidValue;
  if ((!a.scratch && !a.counts) || (loop != nbh::kHistLoopScan && loop != nbh::kHistLoopGated)) return (int)hipErrorInvalidValue;
  if (fp64) hist<double>(a); else hist<float>(a);
  return 0;
}
int launch_hist_combine_kernel(hipStream_t, const nbh::HistArgs& a) {
  if (a.m <= 0 || a.n_bins < 1 || a.n_bins > nbh::kHistMaxBins || !a.scratch || !a.counts || a.chunks < 1) return (int)hipErrorInvalidValue;
  g_combines.fetch_add(1);
  for (int p = 0; p < a.m; ++p)
    for (int b = 0; b < a.n_bins; ++b) {
      int v = 0;
      for (int y = 0; y < a.chunks; ++y) v += a.scratch[nbh::hist_scratch_at(a, y, b, p)];
      a.counts[(size_t)p * (size_t)a.n_bins + (size_t)b] = v;
    }
  return 0;
}
int launch_hist_reduce_kernel(hipStream_t, const int* counts, int rows, int n_bins, unsigned long long* sums) {
  if (rows < 0 || n_bins < 1 || n_bins > nbh::kHistMaxBins || !sums || (rows > 0 && !counts)) return (int)hipErrorInvalidValue;
  g_reduces.fetch_add(1);
  for (int r = 0; r < rows; ++r)
    for (int b = 0; b < n_bins; ++b) sums[b] += (unsigned long long)counts[(size_t)r * (size_t)n_bins + (size_t)b];
  return 0;
}
}  // namespace nbl
