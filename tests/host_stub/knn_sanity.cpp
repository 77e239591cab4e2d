// knn_sanity.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): drives nbody_knn_rows and nbody_knn (and their _d forms) of
// the library's host code (knn.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp, point_sums.cpp, neighbors.cpp) against
// tests/host_stub/hip_stub.cpp and knn_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's logic: the rows of a
// window and the division of the points over the devices, the upload and copy-back offsets of [m][k] outputs, the choice of the source
// split, the k-dependent scratch size and the batches, the argument checks, lifetimes at shutdown and the failure paths.  knn_stub.cpp
// states the values expected here.  neighbors_stub.cpp and point_sums_stub.cpp are linked for neighbors.cpp and point_sums.cpp; nbody_nearest
// runs between knn calls on one context (the passes share their query buffers).
#include <math.h>
#include <string.h>

#include <algorithm>

#define SANITY_NAME "knn_sanity"
#include "sanity_common.hpp"

extern "C" long knn_stub_combines(void);   // knn_stub.cpp: combine launches so far, one per batch of a split launch

static void set_env(const char* split, const char* scratch_mb) {
  if (split) setenv("NBODY_KNN_SPLIT", split, 1); else unsetenv("NBODY_KNN_SPLIT");
  if (scratch_mb) setenv("NBODY_KNN_SCRATCH_MB", scratch_mb, 1); else unsetenv("NBODY_KNN_SCRATCH_MB");
}

static int rows(int f, int n, int k, int* i, float* d) { return nbody_knn_rows(f, n, k, i, d); }
static int rows(int f, int n, int k, int* i, double* d) { return nbody_knn_rows_d(f, n, k, i, d); }
static int at(const float* p, int m, const int* sk, int k, int* i, float* d) { return nbody_knn(p, m, sk, k, i, d); }
static int at(const double* p, int m, const int* sk, int k, int* i, double* d) { return nbody_knn_d(p, m, sk, k, i, d); }
static int nearest(const float* p, int m, const int* sk, int* i, float* d) { return nbody_nearest(p, m, sk, i, d, 0.f, nullptr); }
static int nearest(const double* p, int m, const int* sk, int* i, double* d) { return nbody_nearest_d(p, m, sk, i, d, 0.0, nullptr); }

// small integers everywhere: every value of knn_stub.cpp is exact in either precision
template <typename T>
struct Case {
  int n, m;
  std::vector<T> pos, vel, pts, d2;
  std::vector<int> skip, idx;
  Case(int n_, int m_) : n(n_), m(m_), pos((size_t)n_ * 4), vel((size_t)n_ * 4, (T)0), pts((size_t)m_ * 4), d2((size_t)std::max(n_, m_) * NBODY_KNN_MAX + 1),
                         skip((size_t)m_), idx((size_t)std::max(n_, m_) * NBODY_KNN_MAX + 1) {
    for (int j = 0; j < n; ++j) { pos[4 * (size_t)j] = (T)((j * 37) % 101); pos[4 * (size_t)j + 1] = (T)(j % 7); pos[4 * (size_t)j + 2] = (T)1; pos[4 * (size_t)j + 3] = (T)(j % 977); }
    for (int p = 0; p < m; ++p) {
      pts[4 * (size_t)p] = (T)(p % 17); pts[4 * (size_t)p + 1] = (T)(p % 5); pts[4 * (size_t)p + 2] = (T)3; pts[4 * (size_t)p + 3] = (T)p;
      skip[(size_t)p] = p % 3 == 0 ? -1 : (int)(((long long)p * 7919) % n);
    }
  }
  void open(int ngpus) { OK(nbody_init(n, ngpus, sizeof(T) == 8, 0)); OK(upload<T>(pos, vel)); }
  // what knn_stub.cpp makes of a query {x, w} with the excluded body sk: k entries
  void expect(T x, T w, int sk, int k, int* e_idx, T* e_d2) const {
    for (int r = 0; r < k; ++r) { e_idx[r] = -1; e_d2[r] = (T)INFINITY; }
    for (int b = 0; b * 1024 < n; ++b) {
      const int b0 = b * 1024, len = std::min(1024, n - b0), j = b0 + ((int)w + b) % len;
      const T d = pos[4 * (size_t)j] - x, v = d < 0 ? -d : d;
      if (j == sk || !(v < e_d2[k - 1])) continue;
      int r = k - 1;
      for (; r > 0 && v < e_d2[r - 1]; --r) { e_d2[r] = e_d2[r - 1]; e_idx[r] = e_idx[r - 1]; }
      e_d2[r] = v; e_idx[r] = j;
    }
  }
  void verify(int cnt_q, int k, const std::function<void(int, T*, T*, int*)>& query, bool w_idx, bool w_d2) {
    for (int q = 0; q < cnt_q; ++q) {
      T x, w, e_d2[NBODY_KNN_MAX]; int sk, e_idx[NBODY_KNN_MAX];
      query(q, &x, &w, &sk);
      expect(x, w, sk, k, e_idx, e_d2);
      for (int r = 0; r < k; ++r) {
        CHECK(idx[(size_t)q * k + r] == (w_idx ? e_idx[r] : -77));
        CHECK(d2[(size_t)q * k + r] == (w_d2 ? e_d2[r] : (T)-77));
      }
    }
    for (size_t e = (size_t)cnt_q * k; e < idx.size(); ++e) CHECK(idx[e] == -77 && d2[e] == (T)-77);   // nothing beyond
  }
  void mark() { std::fill(idx.begin(), idx.end(), -77); std::fill(d2.begin(), d2.end(), (T)-77); }
  void run_rows(int first, int count, int k, bool w_idx, bool w_d2) {
    mark();
    OK(rows(first, count, k, w_idx ? idx.data() : nullptr, w_d2 ? d2.data() : nullptr));
    verify(count, k, [&](int q, T* x, T* w, int* sk) { *x = pos[4 * (size_t)(first + q)]; *w = pos[4 * (size_t)(first + q) + 3]; *sk = first + q; }, w_idx, w_d2);
  }
  void run_points(bool with_skip, int k, bool w_idx, bool w_d2, int p0 = 0, int count = -1) {
    if (count < 0) count = m - p0;
    mark();
    OK(at(pts.data() + 4 * (size_t)p0, count, with_skip ? skip.data() + p0 : nullptr, k, w_idx ? idx.data() : nullptr, w_d2 ? d2.data() : nullptr));
    verify(count, k, [&](int q, T* x, T* w, int* sk) { *x = pts[4 * (size_t)(p0 + q)]; *w = pts[4 * (size_t)(p0 + q) + 3]; *sk = with_skip ? skip[(size_t)(p0 + q)] : -1; },
           w_idx, w_d2);
  }
  // nbody_nearest at the first `count` points equals entry 0 of the knn stub's list (both stubs offer the same candidates)
  void run_nearest(int count) {
    std::vector<int> ni((size_t)count + 1, -77);
    std::vector<T> nd((size_t)count + 1, (T)-77);
    OK(nearest(pts.data(), count, skip.data(), ni.data(), nd.data()));
    for (int q = 0; q < count; ++q) {
      int e_idx; T e_d2;
      expect(pts[4 * (size_t)q], pts[4 * (size_t)q + 3], skip[(size_t)q], 1, &e_idx, &e_d2);
      CHECK(ni[(size_t)q] == e_idx && nd[(size_t)q] == e_d2);
    }
    CHECK(ni[(size_t)count] == -77 && nd[(size_t)count] == (T)-77);
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
  for (int m : {1, 255, 256, 257, 5000}) {
    Case<T> c(n, m);
    c.open(ngpus);
    for (const char* split : {(const char*)nullptr, "0", "1", "3", "1000"}) {
      set_env(split, nullptr);
      c.run_all();
    }
    set_env(nullptr, nullptr);
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
    set_env("3", "0.06");
    const long before = knn_stub_combines();
    c.run_points(true, 5, true, true, 0, 700);
    CHECK(knn_stub_combines() - before == batches);
    set_env(nullptr, nullptr);
    c.run_nearest(257);
    c.run_points(true, 32, true, true);
    c.run_nearest(5000);
    c.run_points(true, 1, true, true);
  }
  SHUTDOWN();
}

int main() {
  const bool three_devices = getenv("STUB_DEVICES") && atoi(getenv("STUB_DEVICES")) >= 3;
  {
    float one[4] = {0, 0, 0, 0}, d[2] = {5, 5};
    double oned[4] = {0, 0, 0, 0}, dd[2] = {5, 5};
    int i[2] = {5, 5};
    CHECK(nbody_knn_rows(0, 1, 2, i, d) == NBODY_ERR_NOT_INIT && nbody_knn_rows_d(0, 1, 2, i, dd) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_knn(one, 1, nullptr, 2, i, d) == NBODY_ERR_NOT_INIT && nbody_knn_d(oned, 1, nullptr, 2, i, dd) == NBODY_ERR_NOT_INIT);
    CHECK(i[0] == 5 && i[1] == 5 && d[0] == 5 && d[1] == 5 && dd[0] == 5 && dd[1] == 5);
  }

  // ---- one block, six blocks with a short last one; one device and three with ragged slices (5200 = 1733 + 1733 + 1734, 1000 = 333 + 333 + 334) ----
  for (int n : {1, 1000, 5200}) {
    shapes<float>(n, 1);
    if (three_devices && n >= 3) shapes<float>(n, 3);
  }
  shapes<double>(5200, 1);
  if (three_devices) shapes<double>(1000, 3);

  // ---- the batched path: 5000 queries x 6 chunks x k x 8 B (k = 32: 7.7 MB) against 0.05 MB: k = 1 (48 B a query) in batches of 1024,
  //      k = 5 (240 B: 218 fit) and k = 32 (1536 B: 34 fit) not one workgroup, hence unsplit; against 1 MB: k = 5 in batches of 4352,
  //      k = 32 in batches of 512 ----
  for (int ngpus : {1, 3}) {
    if (ngpus > 1 && !three_devices) continue;
    Case<float> c(5200, 5000);
    c.open(ngpus);
    for (const char* mb : {"0.05", "1"})
      for (const char* split : {(const char*)nullptr, "4", "6"}) {
        set_env(split, mb);
        const long before = knn_stub_combines();
        c.run_all();
        CHECK(knn_stub_combines() > before);
      }
    set_env(nullptr, "0");    // not one workgroup's queries fit: no split
    long before = knn_stub_combines();
    c.run_all();
    set_env("5", "0");
    c.run_all();
    CHECK(knn_stub_combines() == before);
    SHUTDOWN();
  }
  {
    Case<double> c(5200, 1000);
    c.open(1);
    set_env(nullptr, "0.3");
    c.run_all();
    SHUTDOWN();
  }
  set_env(nullptr, nullptr);

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(5200, 300);
    c.open(three_devices ? 3 : 1);
    float* pts = c.pts.data();
    c.mark();
    int* I = c.idx.data(); float* D = c.d2.data();
    CHECK(nbody_knn_rows(0, 300, 5, nullptr, nullptr) == NBODY_ERR_ARG);
    for (int k : {0, -1, NBODY_KNN_MAX + 1, 1 << 30}) {
      CHECK(nbody_knn_rows(0, 300, k, I, D) == NBODY_ERR_ARG);
      CHECK(nbody_knn(pts, 300, nullptr, k, I, D) == NBODY_ERR_ARG);
    }
    CHECK(nbody_knn_rows(-1, 300, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn_rows(0, 0, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn_rows(0, -4, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn_rows(5200, 1, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn_rows(5000, 201, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn_rows(1 << 30, 1 << 30, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn(nullptr, 300, nullptr, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn(pts, 0, nullptr, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn(pts, -1, nullptr, 5, I, D) == NBODY_ERR_ARG);
    CHECK(nbody_knn(pts, 300, nullptr, 5, nullptr, nullptr) == NBODY_ERR_ARG);
    for (int bad : {5200, -2, 1 << 30}) {
      std::vector<int> sk = c.skip;
      sk[299] = bad;
      CHECK(nbody_knn(pts, 300, sk.data(), 5, I, D) == NBODY_ERR_ARG);
    }
    std::vector<double> pd(1200, 0.0), dd(1500, 5.0);
    CHECK(nbody_knn_d(pd.data(), 300, nullptr, 5, I, dd.data()) == NBODY_ERR_STATE);
    CHECK(nbody_knn_rows_d(0, 300, 5, I, dd.data()) == NBODY_ERR_STATE);
    CHECK(dd[0] == 5.0 && dd[1499] == 5.0);
    for (size_t e = 0; e < c.idx.size(); ++e) CHECK(c.idx[e] == -77 && c.d2[e] == -77.f);
    std::vector<int> edge = c.skip;
    edge[0] = 5199; edge[299] = 0;
    OK(nbody_knn(pts, 300, edge.data(), 5, I, nullptr));
    CHECK(c.d2[0] == -77.f && c.idx[0] != -77);
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_knn(pts, 10, nullptr, 5, I, D) == NBODY_ERR_STATE && nbody_knn_rows(0, 10, 5, I, D) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the buffers shared with the neighbour pass ----
  for (int ngpus : {1, 3}) {
    if (ngpus > 1 && !three_devices) continue;
    interleaved<float>(ngpus);
    interleaved<double>(ngpus);
  }

  // ---- the failure paths: every allocating call of a call, one device and three, split (scratch) and not ----
  for (int ngpus : {1, 3}) {
    if (ngpus > 1 && !three_devices) continue;
    Case<float> c(5200, 700);
    set_env("3", nullptr);
    int made = sweep("nbody_knn split", [&] { c.open(ngpus); }, [&] { return nbody_knn(c.pts.data(), c.m, c.skip.data(), 5, c.idx.data(), c.d2.data()); },
                     [&] { c.run_points(true, 5, true, true); });
    CHECK(made == 5 * ngpus);   // points, skip, idx, d2, scratch per device
    made = sweep("nbody_knn_rows split", [&] { c.open(ngpus); }, [&] { return nbody_knn_rows(0, 5200, 32, c.idx.data(), c.d2.data()); },
                 [&] { c.run_rows(0, 5200, 32, true, true); });
    CHECK(made == 3 * ngpus);   // idx, d2, scratch
    set_env("1", nullptr);
    made = sweep("nbody_knn", [&] { c.open(ngpus); }, [&] { return nbody_knn(c.pts.data(), c.m, nullptr, 1, nullptr, c.d2.data()); },
                 [&] { c.run_points(false, 1, false, true); });
    CHECK(made == 2 * ngpus);   // points, d2
  }
  set_env(nullptr, nullptr);
  printf("knn_sanity ok\n");
  return 0;
}
