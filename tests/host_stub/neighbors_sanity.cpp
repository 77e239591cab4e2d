// neighbors_sanity.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): drives nbody_neighbors_rows, nbody_nearest and
// nbody_closest_pair (and their _d forms) of the library's host code (neighbors.cpp beside context.cpp, comm.cpp, mailbox.cpp,
// energy.cpp) against tests/host_stub/hip_stub.cpp and neighbors_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's
// logic: the rows of a window and the division of the points over the devices, the upload and copy-back offsets, the choice of the
// source split, the scratch size and the batches, the argument checks, the closest pair over the devices, lifetimes at shutdown and
// the failure paths.  neighbors_stub.cpp states the values expected here.  point_sums.cpp and point_sums_stub.cpp are linked too, for the
// nbody_field calls between neighbour calls on one context (the two passes share their query buffers).
#include <math.h>
#include <string.h>

#define SANITY_NAME "neighbors_sanity"
#include "sanity_common.hpp"

extern "C" long neighbors_stub_combines(void);   // neighbors_stub.cpp: combine launches so far, one per batch of a split launch

static const SplitEnv env = {"NBODY_NEIGHBORS_SPLIT", "NBODY_NEIGHBORS_SCRATCH_MB"};

static int rows(int f, int n, int* i, float* d, float r2, int* c) { return nbody_neighbors_rows(f, n, i, d, r2, c); }
static int rows(int f, int n, int* i, double* d, double r2, int* c) { return nbody_neighbors_rows_d(f, n, i, d, r2, c); }
static int nearest(const float* p, int m, const int* sk, int* i, float* d, float r2, int* c) { return nbody_nearest(p, m, sk, i, d, r2, c); }
static int nearest(const double* p, int m, const int* sk, int* i, double* d, double r2, int* c) { return nbody_nearest_d(p, m, sk, i, d, r2, c); }
static int pair(int* i, int* j, float* d) { return nbody_closest_pair(i, j, d); }
static int pair(int* i, int* j, double* d) { return nbody_closest_pair_d(i, j, d); }
static int field(const float* p, int m, const int* sk, float* a, float* phi) { return nbody_field(p, m, sk, a, phi); }
static int field(const double* p, int m, const int* sk, double* a, double* phi) { return nbody_field_d(p, m, sk, a, phi); }

template <typename T>
struct Case : Fixture<T> {
  using F = Fixture<T>;
  using Q = typename F::Q;
  using F::n; using F::m; using F::pos; using F::pts; using F::skip;
  std::vector<T> d2;
  std::vector<int> idx, cnt;
  Case(int n_, int m_) : F(n_, m_), d2((size_t)std::max(n_, m_)), idx((size_t)std::max(n_, m_)), cnt((size_t)std::max(n_, m_)) {}
  // what neighbors_stub.cpp makes of a query
  void expect(const Q& q, T r2, int* e_idx, T* e_d2, int* e_cnt) const {
    *e_idx = -1; *e_d2 = (T)INFINITY; *e_cnt = 0;
    for (int b = 0; b < stub::blocks_of(n); ++b) {
      const auto [j, b0, len] = stub::candidate(n, q.w, b);
      const T v = stub::absdiff(pos[4 * (size_t)j], q.x);
      if (j != q.sk && v < *e_d2) { *e_d2 = v; *e_idx = j; }
      if ((T)b <= r2) *e_cnt += len - (q.sk >= b0 && q.sk < b0 + len ? 1 : 0);
    }
  }
  void verify(int cnt_q, const std::function<Q(int)>& query, T r2, bool w_idx, bool w_d2, bool w_cnt) {
    for (int k = 0; k < cnt_q; ++k) {
      T e_d2; int e_idx, e_cnt;
      expect(query(k), r2, &e_idx, &e_d2, &e_cnt);
      CHECK(idx[(size_t)k] == (w_idx ? e_idx : kMark));
      CHECK(d2[(size_t)k] == (w_d2 ? e_d2 : (T)kMark));
      CHECK(cnt[(size_t)k] == (w_cnt ? e_cnt : kMark));
    }
    CHECK(nothing_beyond(idx, (size_t)cnt_q) && nothing_beyond(d2, (size_t)cnt_q) && nothing_beyond(cnt, (size_t)cnt_q));
  }
  void mark_all() { mark(idx); mark(d2); mark(cnt); }
  void run_rows(int first, int count, bool w_idx, bool w_d2, bool w_cnt, T r2) {
    mark_all();
    OK(rows(first, count, w_idx ? idx.data() : nullptr, w_d2 ? d2.data() : nullptr, r2, w_cnt ? cnt.data() : nullptr));
    verify(count, [&](int k) { return this->row(first + k); }, r2, w_idx, w_d2, w_cnt);
  }
  void run_points(bool with_skip, bool w_idx, bool w_d2, bool w_cnt, T r2, int p0 = 0, int count = -1) {
    if (count < 0) count = m - p0;
    mark_all();
    OK(nearest(pts.data() + 4 * (size_t)p0, count, with_skip ? skip.data() + p0 : nullptr, w_idx ? idx.data() : nullptr, w_d2 ? d2.data() : nullptr, r2,
               w_cnt ? cnt.data() : nullptr));
    verify(count, [&](int k) { return this->point(p0 + k, with_skip); }, r2, w_idx, w_d2, w_cnt);
  }
  void run_pair() {
    int bi = -1, bj = -1; T bd = (T)INFINITY;
    for (int r = 0; r < n; ++r) {
      int e_idx, e_cnt; T e_d2;
      expect(this->row(r), (T)0, &e_idx, &e_d2, &e_cnt);
      if (e_d2 < bd) { bd = e_d2; bi = r; bj = e_idx; }
    }
    int i = -5, j = -5; T d = (T)-5;
    OK(pair(&i, &j, &d));
    CHECK(i == bi && j == bj && d == bd);
    int j2 = -5;
    OK(pair(nullptr, &j2, (T*)nullptr));
    CHECK(j2 == bj);
  }
  // nbody_field at the first `count` points, with skip, against what point_sums_stub.cpp makes of them
  void run_field(int count) {
    std::vector<T> acc((size_t)count * 4 + 4, (T)kMark), phi((size_t)count + 1, (T)kMark);
    OK(field(pts.data(), count, skip.data(), acc.data(), phi.data()));
    const int nb = stub::blocks_of(n);
    for (int p = 0; p < count; ++p) {
      double ax = 0.0, ay = 0.0, az = 0.0;
      for (int b = 0; b < nb; ++b) {
        ax += (double)(T)(pos[4 * (size_t)b * stub::kBlock] - pts[4 * (size_t)p]);
        ay += (double)(T)(pts[4 * (size_t)p + 1] + (T)b);
        az += (double)(T)((T)skip[(size_t)p] + (b == nb - 1 ? pos[4 * (size_t)(n - 1)] : (T)0));
      }
      CHECK(acc[4 * (size_t)p] == (T)ax && acc[4 * (size_t)p + 1] == (T)ay && acc[4 * (size_t)p + 2] == (T)az && acc[4 * (size_t)p + 3] == (T)0);
      CHECK(phi[(size_t)p] == (T)(0.0 - (double)nb * (double)p));
    }
    CHECK(nothing_beyond(acc, 4 * (size_t)count) && nothing_beyond(phi, (size_t)count));
  }
  void run_all() {
    run_points(false, true, true, true, (T)1);
    run_points(true, true, true, true, (T)0);
    run_points(true, false, true, false, (T)0);
    run_points(false, true, false, false, (T)0);
    run_points(true, false, false, true, (T)2);
    if (m > 2) run_points(true, true, true, true, (T)1, 1, m - 2);
    const int rc = std::min(m, n);   // the row counts are the point counts, as far as there are rows
    run_rows(0, rc, true, true, true, (T)1);
    run_rows(n - rc, rc, true, true, false, (T)0);
    run_rows((n - rc) / 2, rc, false, true, true, (T)0);   // a window in the middle: across the devices when there are three
    run_rows((n - rc) / 2, rc, true, false, false, (T)0);
    run_rows(n - 1, 1, false, false, true, (T)5);
  }
};

template <typename T>
static void shapes(int n, int ngpus) {
  for (int m : kShapeM) {
    Case<T> c(n, m);
    c.open(ngpus);
    for_splits(env, {nullptr, "0", "1", "2", "3", "1000"}, [&] { c.run_all(); });
    c.run_pair();
    SHUTDOWN();
  }
}

// The field pass between neighbour calls on one context: both keep their points, skip indices and split scratch in the Local's q_*
// buffers (query_pass.hpp), so each call meets buffers the other pass sized.  N = 2100: three blocks, a tail that is no multiple of 64.
// m = 700 over three chunks against 0.02 MB = 20971 B of scratch.  One device: fp32 takes 36 B a query, 582 fit, batches of 512 + 188;
// fp64 takes 48 B, 436 fit, batches of 256 + 256 + 188.  Three devices: 233 or 234 queries each, fewer than one workgroup's 256, so
// each device's queries go as one split batch (a bound that cut them would fit no whole workgroup, which means no split at all).
// The count of combine launches (one per split batch) says that the split and the batches happened.  Then m = 257 field points (85
// or 86 a device; their per-block sums are the larger scratch) and m = 5000.
template <typename T>
static void interleaved(int ngpus) {
  unsetenv("NBODY_FIELD_SPLIT"); unsetenv("NBODY_FIELD_SCRATCH_MB");
  Case<T> c(2100, 5000);
  c.open(ngpus);
  const long batches = ngpus > 1 ? ngpus : sizeof(T) == 4 ? 2 : 3;
  for (int round = 0; round < 2; ++round) {
    env.set("3", "0.02");
    const long before = neighbors_stub_combines();
    c.run_points(true, true, true, true, (T)1, 0, 700);
    CHECK(neighbors_stub_combines() - before == batches);
    env.set(nullptr, nullptr);
    c.run_field(257);
    c.run_points(true, true, true, true, (T)1);
  }
  SHUTDOWN();
}

int main() {
  {
    float one[4] = {0, 0, 0, 0}, d[1] = {5};
    double oned[4] = {0, 0, 0, 0}, dd[1] = {5};
    int i[2] = {5, 5}, c[1] = {5};
    CHECK(nbody_neighbors_rows(0, 1, i, d, 1.f, c) == NBODY_ERR_NOT_INIT && nbody_neighbors_rows_d(0, 1, i, dd, 1.0, c) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_nearest(one, 1, nullptr, i, d, 1.f, c) == NBODY_ERR_NOT_INIT && nbody_nearest_d(oned, 1, nullptr, i, dd, 1.0, c) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_closest_pair(i, i + 1, d) == NBODY_ERR_NOT_INIT && nbody_closest_pair_d(i, i + 1, dd) == NBODY_ERR_NOT_INIT);
    CHECK(i[0] == 5 && i[1] == 5 && c[0] == 5 && d[0] == 5 && dd[0] == 5);
  }

  // ---- one block, six blocks with a short last one; one device and three with ragged slices (5200 = 1733 + 1733 + 1734, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 1000, 5200}, shapes<float>, shapes<double>);

  // ---- the batched path: 5000 queries x 6 chunks x 12 B = 360 kB against 0.05 MB: batches of 512 (fp32), of 512 at 16 B too (fp64) ----
  for_device_counts([](int ngpus) {
    Case<float> c(5200, 5000);
    c.open(ngpus);
    for (const char* split : {(const char*)nullptr, "4", "6"}) {
      env.set(split, "0.05");
      c.run_all();
    }
    env.set(nullptr, "0");    // not one workgroup's queries fit: no split
    c.run_all();
    env.set("5", "0");
    c.run_all();
    env.set(nullptr, "0.05");
    c.run_pair();
    SHUTDOWN();
  });
  {
    Case<double> c(5200, 1000);
    c.open(1);
    env.set(nullptr, "0.05");
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
    int* I = c.idx.data(); float* D = c.d2.data(); int* N = c.cnt.data();
    CHECK(nbody_neighbors_rows(0, 300, nullptr, nullptr, 1.f, nullptr) == NBODY_ERR_ARG);
    for (const Window& w : refused_windows(5200, 300)) CHECK(nbody_neighbors_rows(w.first, w.count, I, D, 1.f, N) == NBODY_ERR_ARG);
    CHECK(nbody_nearest(nullptr, 300, nullptr, I, D, 1.f, N) == NBODY_ERR_ARG);
    CHECK(nbody_nearest(pts, 0, nullptr, I, D, 1.f, N) == NBODY_ERR_ARG);
    CHECK(nbody_nearest(pts, -1, nullptr, I, D, 1.f, N) == NBODY_ERR_ARG);
    CHECK(nbody_nearest(pts, 300, nullptr, nullptr, nullptr, 1.f, nullptr) == NBODY_ERR_ARG);
    for (int bad : refused_skips(5200)) CHECK(nbody_nearest(pts, 300, c.skip_with(299, bad).data(), I, D, 1.f, N) == NBODY_ERR_ARG);
    CHECK(nbody_closest_pair(nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    std::vector<double> pd(1200, 0.0), dd(300, 5.0);
    CHECK(nbody_nearest_d(pd.data(), 300, nullptr, I, dd.data(), 1.0, N) == NBODY_ERR_STATE);
    CHECK(nbody_neighbors_rows_d(0, 300, I, dd.data(), 1.0, N) == NBODY_ERR_STATE && nbody_closest_pair_d(I, I + 1, dd.data()) == NBODY_ERR_STATE);
    CHECK(dd[0] == 5.0 && dd[299] == 5.0);
    CHECK(nothing_beyond(c.idx, 0) && nothing_beyond(c.d2, 0) && nothing_beyond(c.cnt, 0));
    std::vector<int> edge = c.skip;
    edge[0] = 5199; edge[299] = 0;
    OK(nbody_nearest(pts, 300, edge.data(), I, nullptr, 1.f, nullptr));
    CHECK(c.d2[0] == (float)kMark && c.cnt[0] == kMark && c.idx[0] != kMark);
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_nearest(pts, 10, nullptr, I, D, 1.f, N) == NBODY_ERR_STATE && nbody_neighbors_rows(0, 10, I, D, 1.f, N) == NBODY_ERR_STATE);
    CHECK(nbody_closest_pair(I, I + 1, D) == NBODY_ERR_STATE);
    d.run_all();
    d.run_pair();
    SHUTDOWN();
  }

  // ---- the buffers shared with the field pass ----
  for_device_counts([](int ngpus) {
    interleaved<float>(ngpus);
    interleaved<double>(ngpus);
  });

  // ---- the failure paths: every allocating call of a call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(5200, 700);
    env.set("3", nullptr);
    int made = sweep("nbody_nearest split", [&] { c.open(ngpus); }, [&] { return nbody_nearest(c.pts.data(), c.m, c.skip.data(), c.idx.data(), c.d2.data(), 1.f, c.cnt.data()); },
                     [&] { c.run_points(true, true, true, true, 1.f); });
    CHECK(made == 6 * ngpus);   // points, skip, idx, d2, count, scratch per device
    made = sweep("nbody_neighbors_rows split", [&] { c.open(ngpus); }, [&] { return nbody_neighbors_rows(0, 5200, c.idx.data(), c.d2.data(), 1.f, nullptr); },
                 [&] { c.run_rows(0, 5200, true, true, false, 1.f); });
    CHECK(made == 3 * ngpus);   // idx, d2, scratch
    env.set("1", nullptr);
    made = sweep("nbody_nearest", [&] { c.open(ngpus); }, [&] { return nbody_nearest(c.pts.data(), c.m, nullptr, nullptr, c.d2.data(), 1.f, nullptr); },
                 [&] { c.run_points(false, false, true, false, 1.f); });
    CHECK(made == 2 * ngpus);   // points, d2
    int i, j; float d;
    made = sweep("nbody_closest_pair", [&] { c.open(ngpus); }, [&] { return nbody_closest_pair(&i, &j, &d); }, [&] { c.run_pair(); });
    CHECK(made == 3 * ngpus);   // idx, d2, the best pairs
  });
  env.set(nullptr, nullptr);
  printf("neighbors_sanity ok\n");
  return 0;
}
