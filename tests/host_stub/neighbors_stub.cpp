// neighbors_stub.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): a host-only stand-in for the launch functions of
// neighbors.hip, linked beside hip_stub.cpp so that neighbors.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.
// hip_stub.cpp's streams are synchronous and the neighbour pass is never captured, so all three functions execute at launch.
// The stand-in pushes values a test can predict through the REAL NeighborsArgs — chunk bounds, the chunks' scratch layout, the combine's
// ascending strict <, pointers the host offset per local and per batch, the rows form's first — so ASan sees every offset the host
// computed.  Per query p (stub_common.hpp: the word q and the excluded body sk) every block b offers the ONE candidate of stub_rule.hpp
// (j_b, d2_b; none if j_b == sk) and
//   count_b = len_b, less one if sk lies in b, when (T)b <= r2, else 0
// taken in ascending b with strict <, counts added.  It says nothing about the kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include <limits>

#include "../../mini_nbody_amd/csrc/neighbors_args.hpp"
#include "stub_common.hpp"

namespace {

using namespace nbn;

template <typename T>
struct Near { T best; int idx, cnt; };

template <typename T>
void block(const NeighborsArgs& a, int p, int b, Near<T>& c) {
  const auto [q, sk] = stub::query_of<T>(a, p);
  const auto [j, b0, len] = stub::candidate(a.n_src, q.w, b);
  const T d2 = stub::absdiff(((const stub::W4<T>*)a.src)[j].x, q.x);
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
  stub::for_each_chunk(a, [&](int p, int y, int b0, int b1) {
    Near<T> c = {std::numeric_limits<T>::infinity(), -1, 0};
    for (int b = b0; b < b1; ++b) block<T>(a, p, b, c);
    if (a.scratch) {
      const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
      ((T*)scratch_d2(a))[w] = c.best;
      scratch_idx(a, sizeof(T))[w] = c.idx;
      if (a.count) scratch_count(a, sizeof(T))[w] = c.cnt;
    } else {
      store<T>(a, p, c);
    }
  });
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

}  // namespace

// combine launches so far: one per batch of a split launch, none when the sources are not split
STUB_COUNTER(neighbors_stub_combines)

namespace nbl {
int launch_neighbors_kernel(int fp64, int loop, hipStream_t, const nbn::NeighborsArgs& a) {
  if (nbd::bad_source_split(a, !a.points)) return (int)hipErrorInvalidValue;
  if (loop != nbn::kNbLoopScan && loop != nbn::kNbLoopWindow) return (int)hipErrorInvalidValue;   // the stub's own: the host passes no other
  if (fp64) neighbors<double>(a); else neighbors<float>(a);
  return 0;
}
int launch_neighbors_combine_kernel(int fp64, hipStream_t, const nbn::NeighborsArgs& a) {
  if (nbd::bad_combine(a)) return (int)hipErrorInvalidValue;
  g_neighbors_stub_combines.fetch_add(1);
  if (fp64) combine<double>(a); else combine<float>(a);
  return 0;
}
int launch_neighbors_best_kernel(int fp64, hipStream_t, const void* d2, const int* idx, int rows, int first, nbn::BestPair* out) {
  if (nbd::bad_row_reduce(rows, out, d2 && idx)) return (int)hipErrorInvalidValue;
  if (fp64) best<double>((const double*)d2, idx, rows, first, out); else best<float>((const float*)d2, idx, rows, first, out);
  return 0;
}
}  // namespace nbl
