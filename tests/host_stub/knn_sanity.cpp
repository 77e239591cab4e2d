// knn_sanity.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): drives nbody_knn_rows and nbody_knn (and their _d forms) of
// the library's host code (knn.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp, point_sums.cpp, neighbors.cpp) against
// tests/host_stub/hip_stub.cpp and knn_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's logic: the rows of a
// window and the division of the points over the devices, the upload and copy-back offsets of [m][k] outputs, the choice of the source
// split, the k-dependent scratch size and the batches, the argument checks, lifetimes at shutdown and the failure paths.  knn_stub.cpp
// states the values expected here.  neighbors_stub.cpp and point_sums_stub.cpp are linked for neighbors.cpp and point_sums.cpp; nbody_nearest
// runs between knn calls on one context (the passes share their query buffers).
#include <math.h>
#include <string.h>

#define SANITY_NAME "knn_sanity"
#include "sanity_common.hpp"

extern "C" long knn_stub_combines(void);   // knn_stub.cpp: combine launches so far, one per batch of a split launch

static const SplitEnv env = {"NBODY_KNN_SPLIT", "NBODY_KNN_SCRATCH_MB"};

static int rows(int f, int n, int k, int* i, float* d) { return nbody_knn_rows(f, n, k, i, d); }
static int rows(int f, int n, int k, int* i, double* d) { return nbody_knn_rows_d(f, n, k, i, d); }
static int at(const float* p, int m, const int* sk, int k, int* i, float* d) { return nbody_knn(p, m, sk, k, i, d); }
static int at(const double* p, int m, const int* sk, int k, int* i, double* d) { return nbody_knn_d(p, m, sk, k, i, d); }
static int nearest(const float* p, int m, const int* sk, int* i, float* d) { return nbody_nearest(p, m, sk, i, d, 0.f, nullptr); }
static int nearest(const double* p, int m, const int* sk, int* i, double* d) { return nbody_nearest_d(p, m, sk, i, d, 0.0, nullptr); }

template <typename T>
struct Case : Fixture<T> {
  using F = Fixture<T>;
  using Q = typename F::Q;
  using F::n; using F::m; using F::pos; using F::pts; using F::skip;
  std::vector<T> d2;
  std::vector<int> idx;
  Case(int n_, int m_) : F(n_, m_), d2((size_t)std::max(n_, m_) * NBODY_KNN_MAX + 1), idx((size_t)std::max(n_, m_) * NBODY_KNN_MAX + 1) {}
  // what knn_stub.cpp makes of a query: k entries
  void expect(const Q& q, int k, int* e_idx, T* e_d2) const {
    for (int r = 0; r < k; ++r) { e_idx[r] = -1; e_d2[r] = (T)INFINITY; }
    for (int b = 0; b < stub::blocks_of(n); ++b) {
      const int j = stub::candidate(n, q.w, b).j;
      const T v = stub::absdiff(pos[4 * (size_t)j], q.x);
      if (j == q.sk || !(v < e_d2[k - 1])) continue;
      int r = k - 1;
      for (; r > 0 && v < e_d2[r - 1]; --r) { e_d2[r] = e_d2[r - 1]; e_idx[r] = e_idx[r - 1]; }
      e_d2[r] = v; e_idx[r] = j;
    }
  }
  void verify(int cnt_q, int k, const std::function<Q(int)>& query, bool w_idx, bool w_d2) {
    for (int q = 0; q < cnt_q; ++q) {
      T e_d2[NBODY_KNN_MAX]; int e_idx[NBODY_KNN_MAX];
      expect(query(q), k, e_idx, e_d2);
      for (int r = 0; r < k; ++r) {
        CHECK(idx[(size_t)q * k + r] == (w_idx ? e_idx[r] : kMark));
        CHECK(d2[(size_t)q * k + r] == (w_d2 ? e_d2[r] : (T)kMark));
      }
    }
    CHECK(nothing_beyond(idx, (size_t)cnt_q * k) && nothing_beyond(d2, (size_t)cnt_q * k));
  }
  void mark_all() { mark(idx); mark(d2); }
  void run_rows(int first, int count, int k, bool w_idx, bool w_d2) {
    mark_all();
    OK(rows(first, count, k, w_idx ? idx.data() : nullptr, w_d2 ? d2.data() : nullptr));
    verify(count, k, [&](int q) { return this->row(first + q); }, w_idx, w_d2);
  }
  void run_points(bool with_skip, int k, bool w_idx, bool w_d2, int p0 = 0, int count = -1) {
    if (count < 0) count = m - p0;
    mark_all();
    OK(at(pts.data() + 4 * (size_t)p0, count, with_skip ? skip.data() + p0 : nullptr, k, w_idx ? idx.data() : nullptr, w_d2 ? d2.data() : nullptr));
    verify(count, k, [&](int q) { return this->point(p0 + q, with_skip); }, w_idx, w_d2);
  }
  // nbody_nearest at the first `count` points equals entry 0 of the knn stub's list (both stubs offer the same candidates)
  void run_nearest(int count) {
    std::vector<int> ni((size_t)count + 1, kMark);
    std::vector<T> nd((size_t)count + 1, (T)kMark);
    OK(nearest(pts.data(), count, skip.data(), ni.data(), nd.data()));
    for (int q = 0; q < count; ++q) {
      int e_idx; T e_d2;
      expect(this->point(q, true), 1, &e_idx, &e_d2);
      CHECK(ni[(size_t)q] == e_idx && nd[(size_t)q] == e_d2);
    }
    CHECK(nothing_beyond(ni, (size_t)count) && nothing_beyond(nd, (size_t)count));
  }
  void run_all() {
    for (int k : {1, 5, 32}) {
      run_points(false, k, true, true);
      run_points(true, k, true, true);
      run_points(true, k, false, true);
      run_points(false, k, true, false);
      if (m > 2) run_points(true, k, true, true, 1, m - 2);
      const int rc = std::min(m, n);   // the row counts are the point counts, as far as there are rows
      run_rows(0, rc, k, true, true);
      run_rows(n - rc, rc, k, true, false);
      run_rows((n - rc) / 2, rc, k, false, true);   // a window in the middle: across the devices when there are three
      run_rows(n - 1, 1, k, true, true);
    }
  }
};

template <typename T>
static void shapes(int n, int ngpus) {
  for (int m : kShapeM) {
    Case<T> c(n, m);
    c.open(ngpus);
    for_splits(env, {nullptr, "0", "1", "3", "1000"}, [&] { c.run_all(); });
    SHUTDOWN();
  }
}

// The neighbour pass between knn calls on one context: both keep their points, skip indices and split scratch in the Local's q_*
// buffers (query_pass.hpp), so each call meets buffers the other pass sized.  N = 2100: three blocks.  m = 700, k = 5 over three chunks
// against 0.06 MB = 62914 B of scratch.  One device: fp32 takes 3 x 5 x 8 = 120 B a query, 524 fit, batches of 512 + 188; fp64 takes
// 180 B, 349 fit, batches of 256 + 256 + 188.  Three devices: 233 or 234 queries each, fewer than one workgroup's 256, so each device's
// queries go as one split batch.  The count of combine launches (one per split batch) says that the split and the batches happened.
template <typename T>
static void interleaved(int ngpus) {
  unsetenv("NBODY_NEIGHBORS_SPLIT"); unsetenv("NBODY_NEIGHBORS_SCRATCH_MB"); unsetenv("NBODY_NEIGHBORS_LOOP");
  Case<T> c(2100, 5000);
  c.open(ngpus);
  const long batches = ngpus > 1 ? ngpus : sizeof(T) == 4 ? 2 : 3;
  for (int round = 0; round < 2; ++round) {
    env.set("3", "0.06");
    const long before = knn_stub_combines();
    c.run_points(true, 5, true, true, 0, 700);
    CHECK(knn_stub_combines() - before == batches);
    env.set(nullptr, nullptr);
    c.run_nearest(257);
    c.run_points(true, 32, true, true);
    c.run_nearest(5000);
    c.run_points(true, 1, true, true);
  }
  SHUTDOWN();
}

int main() {
  {
    float one[4] = {0, 0, 0, 0}, d[2] = {5, 5};
    double oned[4] = {0, 0, 0, 0}, dd[2] = {5, 5};
    int i[2] = {5, 5};
    CHECK(nbody_knn_rows(0, 1, 2, i, d) == NBODY_ERR_NOT_INIT && nbody_knn_rows_d(0, 1, 2, i, dd) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_knn(one, 1, nullptr, 2, i, d) == NBODY_ERR_NOT_INIT && nbody_knn_d(oned, 1, nullptr, 2, i, dd) == NBODY_ERR_NOT_INIT);
    CHECK(i[0] == 5 && i[1] == 5 && d[0] == 5 && d[1] == 5 && dd[0] == 5 && dd[1] == 5);
  }

  // ---- one block, six blocks with a short last one; one device and three with ragged slices (5200 = 1733 + 1733 + 1734, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 1000, 5200}, shapes<float>, shapes<double>);

  // ---- the batched path: 5000 queries x 6 chunks x k x 8 B (k = 32: 7.7 MB) against 0.05 MB: k = 1 (48 B a query) in batches of 1024,
  //      k = 5 (240 B: 218 fit) and k = 32 (1536 B: 34 fit) not one workgroup, hence unsplit; against 1 MB: k = 5 in batches of 4352,
  //      k = 32 in batches of 512 ----
  for_device_counts([](int ngpus) {
    Case<float> c(5200, 5000);
    c.open(ngpus);
    for (const char* mb : {"0.05", "1"})
      for (const char* split : {(const char*)nullptr, "4", "6"}) {
        env.set(split, mb);
        const long before = knn_stub_combines();
        c.run_all();
        CHECK(knn_stub_combines() > before);
      }
    env.set(nullptr, "0");    // not one workgroup's queries fit: no split
    long before = knn_stub_combines();
    c.run_all();
    env.set("5", "0");
    c.run_all();
    CHECK(knn_stub_combines() == before);
    SHUTDOWN();
  });
  {
    Case<double> c(5200, 1000);
    c.open(1);
    env.set(nullptr, "0.3");
    c.run_all();
    SHUTDOWN();
  }
  env.set(nullptr, nullptr);

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(5200, 300);
    c.open(three_devices() ? 3 : 1);
    float* pts = c.pts.data();
    c.mark_all();
    int* I = c.idx.data(); float* D = c.d2.data();
    CHECK(nbody_knn_rows(0, 300, 5, nullptr, nullptr) == NBODY_ERR_ARG);
    for (int k : {0, -1, NBODY_KNN_MAX + 1, 1 << 30}) {
      CHECK(nbody_knn_rows(0, 300, k, I, D) == NBODY_ERR_ARG);
      CHECK(nbody_knn(pts, 300, nullptr, k, I, D) == NBODY_ERR_ARG);
    }
    for (const Window& w : refused_windows(5200, 300)) CHECK(nbody_knn_rows(w.first, w.count, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn(nullptr, 300, nullptr, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn(pts, 0, nullptr, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn(pts, -1, nullptr, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn(pts, 300, nullptr, 5, nullptr, nullptr) == NBODY_ERR_ARG);
    for (int bad : refused_skips(5200)) CHECK(nbody_knn(pts, 300, c.skip_with(299, bad).data(), 5, I, D) == NBODY_ERR_ARG);
    std::vector<double> pd(1200, 0.0), dd(1500, 5.0);
    CHECK(nbody_knn_d(pd.data(), 300, nullptr, 5, I, dd.data()) == NBODY_ERR_STATE);
    CHECK(nbody_knn_rows_d(0, 300, 5, I, dd.data()) == NBODY_ERR_STATE);
    CHECK(dd[0] == 5.0 && dd[1499] == 5.0);
    CHECK(nothing_beyond(c.idx, 0) && nothing_beyond(c.d2, 0));
    std::vector<int> edge = c.skip;
    edge[0] = 5199; edge[299] = 0;
    OK(nbody_knn(pts, 300, edge.data(), 5, I, nullptr));
    CHECK(c.d2[0] == (float)kMark && c.idx[0] != kMark);
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_knn(pts, 10, nullptr, 5, I, D) == NBODY_ERR_STATE && nbody_knn_rows(0, 10, 5, I, D) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the buffers shared with the neighbour pass ----
  for_device_counts([](int ngpus) {
    interleaved<float>(ngpus);
    interleaved<double>(ngpus);
  });

  // ---- the failure paths: every allocating call of a call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(5200, 700);
    env.set("3", nullptr);
    int made = sweep("nbody_knn split", [&] { c.open(ngpus); }, [&] { return nbody_knn(c.pts.data(), c.m, c.skip.data(), 5, c.idx.data(), c.d2.data()); },
                     [&] { c.run_points(true, 5, true, true); });
    CHECK(made == 5 * ngpus);   // points, skip, idx, d2, scratch per device
    made = sweep("nbody_knn_rows split", [&] { c.open(ngpus); }, [&] { return nbody_knn_rows(0, 5200, 32, c.idx.data(), c.d2.data()); },
                 [&] { c.run_rows(0, 5200, 32, true, true); });
    CHECK(made == 3 * ngpus);   // idx, d2, scratch
    env.set("1", nullptr);
    made = sweep("nbody_knn", [&] { c.open(ngpus); }, [&] { return nbody_knn(c.pts.data(), c.m, nullptr, 1, nullptr, c.d2.data()); },
                 [&] { c.run_points(false, 1, false, true); });
    CHECK(made == 2 * ngpus);   // points, d2
  });
  env.set(nullptr, nullptr);
  printf("knn_sanity ok\n");
  return 0;
}
