// knn_stub.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): a host-only stand-in for the launch functions of knn.hip,
// linked beside hip_stub.cpp so that knn.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.  hip_stub.cpp's streams
// are synchronous and the pass is never captured, so both functions execute at launch.
// The stand-in pushes values a test can predict through the REAL KnnArgs — chunk bounds, the chunks' scratch layout [chunk][r][m], the
// combine's stable insertion, pointers the host offset per local and per batch, the [m][k] outputs, the rows form's first — so ASan sees
// every offset the host computed.  Per query p (stub_common.hpp: the word q and the excluded body sk) every block b offers the ONE
// candidate of stub_rule.hpp (j_b, d2_b; none if j_b == sk), as neighbors_stub.cpp's,
// taken in ascending b into a list of k entries from (+inf, -1), each behind every entry with d2 <= its own, the last entry dropped.
// It says nothing about the kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include <limits>

#include "../../mini_nbody_amd/csrc/knn_args.hpp"
#include "stub_common.hpp"

namespace {

using namespace nbq;

template <typename T>
struct List {
  T d[kKnMax];
  int i[kKnMax];
  int k;
  explicit List(int k_) : k(k_) { for (int r = 0; r < k; ++r) { d[r] = std::numeric_limits<T>::infinity(); i[r] = -1; } }
  void push(T v, int j) {
    if (!(v < d[k - 1])) return;
    int r = k - 1;
    for (; r > 0 && v < d[r - 1]; --r) { d[r] = d[r - 1]; i[r] = i[r - 1]; }
    d[r] = v; i[r] = j;
  }
};

template <typename T>
void block(const KnnArgs& a, int p, int b, List<T>& c) {
  const auto [q, sk] = stub::query_of<T>(a, p);
  const int j = stub::candidate(a.n_src, q.w, b).j;
  if (j != sk) c.push(stub::absdiff(((const stub::W4<T>*)a.src)[j].x, q.x), j);
}

template <typename T>
void store(const KnnArgs& a, int p, const List<T>& c) {
  for (int r = 0; r < a.k; ++r) {
    if (a.idx) a.idx[(size_t)p * (size_t)a.k + (size_t)r] = c.i[r];
    if (a.d2) ((T*)a.d2)[(size_t)p * (size_t)a.k + (size_t)r] = c.d[r];
  }
}

template <typename T>
void knn(const KnnArgs& a) {
  stub::for_each_chunk(a, [&](int p, int y, int b0, int b1) {
    List<T> c(a.k);
    for (int b = b0; b < b1; ++b) block<T>(a, p, b, c);
    if (a.scratch) {
      for (int r = 0; r < a.k; ++r) {
        const size_t w = knn_scratch_at(a, y, r, p);
        ((T*)knn_scratch_d2(a))[w] = c.d[r];
        knn_scratch_idx(a, sizeof(T))[w] = c.i[r];
      }
    } else {
      store<T>(a, p, c);
    }
  });
}

template <typename T>
void combine(const KnnArgs& a) {
  for (int p = 0; p < a.m; ++p) {
    List<T> c(a.k);
    for (int y = 0; y < a.chunks; ++y)
      for (int r = 0; r < a.k; ++r) {
        const size_t w = knn_scratch_at(a, y, r, p);
        c.push(((const T*)knn_scratch_d2(a))[w], knn_scratch_idx(a, sizeof(T))[w]);
      }
    store<T>(a, p, c);
  }
}

}  // namespace

// combine launches so far: one per batch of a split launch, none when the sources are not split
STUB_COUNTER(knn_stub_combines)

namespace nbl {
int launch_knn_kernel(int fp64, hipStream_t, const nbq::KnnArgs& a) {
  if (nbq::bad_knn_launch(a)) return (int)hipErrorInvalidValue;
  if (fp64) knn<double>(a); else knn<float>(a);
  return 0;
}
int launch_knn_combine_kernel(int fp64, hipStream_t, const nbq::KnnArgs& a) {
  if (nbq::bad_knn_combine(a)) return (int)hipErrorInvalidValue;
  g_knn_stub_combines.fetch_add(1);
  if (fp64) combine<double>(a); else combine<float>(a);
  return 0;
}
}  // namespace nbl
