// neighbors_stub.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): a host-only stand-in for the launch functions of
// neighbors.hip, linked beside hip_stub.cpp so that neighbors.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.
// hip_stub.cpp's streams are synchronous and the neighbour pass is never captured, so all three functions execute at launch.
// The stand-in pushes values a test can predict through the REAL NeighborsArgs — chunk bounds, the chunks' scratch layout, the combine's
// ascending strict <, pointers the host offset per local and per batch, the rows form's first — so ASan sees every offset the host
// computed.  Per query p (q = points[p], or in the rows form source first + p; sk = skip[p], -1, or in the rows form first + p) every
// block b of 1024 sources (len_b of them) offers ONE candidate:
//   j_b = 1024 b + ((int)q.w + b) mod len_b      d2_b = |src[j_b].x - q.x|      (none if j_b == sk)
//   count_b = len_b, less one if sk lies in b, when (T)b <= r2, else 0
// taken in ascending b with strict <, counts added; q.w, which the real kernel ignores, lets a driver steer the candidates.  It says
// nothing about the kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <limits>

#include "../../mini_nbody_amd/csrc/neighbors_args.hpp"

namespace {

using namespace nbn;

template <typename T>
struct W4 { T x, y, z, w; };

template <typename T>
struct Near { T best; int idx, cnt; };

template <typename T>
void block(const NeighborsArgs& a, int p, int b, Near<T>& c) {
  typedef W4<T> V;
  const V* src = (const V*)a.src;
  const V q = a.points ? ((const V*)a.points)[p] : src[a.first + p];
  const int sk = a.points ? (a.skip ? a.skip[p] : -1) : a.first + p;
  const int b0 = b * nbd::kSrcBlock, len = std::min(nbd::kSrcBlock, a.n_src - b0);
  const int j = b0 + ((int)q.w + b) % len;
  const T d = src[j].x - q.x, d2 = d < 0 ? -d : d;
  if (j != sk && d2 < c.best) { c.best = d2; c.idx = j; }
  if (a.count && (T)b <= (T)a.r2) c.cnt += len - (sk >= b0 && sk < b0 + len ? 1 : 0);
}

template <typename T>
void store(const NeighborsArgs& a, int p, const Near<T>& c) {
  if (a.idx) a.idx[p] = c.idx;
  if (a.d2) ((T*)a.d2)[p] = c.best;
  if (a.count) a.count[p] = c.cnt;
}

template <typename T>
void neighbors(const NeighborsArgs& a) {
  for (int p = 0; p < a.m; ++p)
    for (int y = 0; y < a.chunks; ++y) {
      Near<T> c = {std::numeric_limits<T>::infinity(), -1, 0};
      const int blk1 = std::min((y + 1) * a.chunk_blocks, a.n_blocks);
      for (int b = y * a.chunk_blocks; b < blk1; ++b) block<T>(a, p, b, c);
      if (a.scratch) {
        const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
        ((T*)scratch_d2(a))[w] = c.best;
        scratch_idx(a, sizeof(T))[w] = c.idx;
        if (a.count) scratch_count(a, sizeof(T))[w] = c.cnt;
      } else {
        store<T>(a, p, c);
      }
    }
}

template <typename T>
void combine(const NeighborsArgs& a) {
  for (int p = 0; p < a.m; ++p) {
    Near<T> c = {std::numeric_limits<T>::infinity(), -1, 0};
    for (int y = 0; y < a.chunks; ++y) {
      const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
      const T d2 = ((const T*)scratch_d2(a))[w];
      if (d2 < c.best) { c.best = d2; c.idx = scratch_idx(a, sizeof(T))[w]; }
      if (a.count) c.cnt += scratch_count(a, sizeof(T))[w];
    }
    store<T>(a, p, c);
  }
}

template <typename T>
void best(const T* d2, const int* idx, int rows, int first, BestPair* out) {
  BestPair b = {std::numeric_limits<double>::infinity(), -1, -1};
  for (int r = 0; r < rows; ++r)
    if ((double)d2[r] < b.d2) { b.d2 = (double)d2[r]; b.i = first + r; b.j = idx[r]; }
  *out = b;
}

std::atomic<long> g_combines{0};

}  // namespace

// combine launches so far: one per batch of a split launch, none when the sources are not split
extern "C" long neighbors_stub_combines(void) { return g_combines.load(); }

namespace nbl {
int launch_neighbors_kernel(int fp64, int loop, hipStream_t, const nbn::NeighborsArgs& a) {
  if (nbd::bad_source_split(a, !a.points)) return (int)hipErrorInvalidValue;
  if (loop != nbn::kNbLoopScan && loop != nbn::kNbLoopWindow) return (int)hipErrorInvalidValue;
  if (fp64) neighbors<double>(a); else neighbors<float>(a);
  return 0;
}
int launch_neighbors_combine_kernel(int fp64, hipStream_t, const nbn::NeighborsArgs& a) {
  if (a.m <= 0 || !a.scratch || a.chunks < 1) return (int)hipErrorInvalidValue;
  g_combines.fetch_add(1);
  if (fp64) combine<double>(a); else combine<float>(a);
  return 0;
}
int launch_neighbors_best_kernel(int fp64, hipStream_t, const void* d2, const int* idx, int rows, int first, nbn::BestPair* out) {
  if (rows < 0 || !out || (rows > 0 && (!d2 || !idx))) return (int)hipErrorInvalidValue;
  if (fp64) best<double>((const double*)d2, idx, rows, first, out); else best<float>((const float*)d2, idx, rows, first, out);
  return 0;
}
}  // namespace nbl
