// hist_sanity.cpp — TEST INFRASTRUCTURE (tests/test_hist_host_sanitizers.py): drives nbody_radial_counts_rows, nbody_radial_counts and
// nbody_pair_histogram (and their _d forms) of the library's host code (hist.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp,
// neighbors.cpp) against tests/host_stub/hip_stub.cpp and hist_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's
// logic: the edge slots, the rows of a window and the division of the points over the devices, the upload and copy-back offsets of
// [m][n_bins] outputs, the choice of the source split, the n_bins-dependent scratch size and the batches, the batches of rows of the
// pair histogram and the sum over the devices, the argument checks, lifetimes at shutdown and the failure paths.  hist_stub.cpp states
// the values expected here.  neighbors_stub.cpp is linked for neighbors.cpp; nbody_nearest runs between histogram calls on one context
// (the passes share their query buffers).
#include <math.h>
#include <string.h>

#include <algorithm>

#define SANITY_NAME "hist_sanity"
#include "sanity_common.hpp"

extern "C" long hist_stub_combines(void);   // hist_stub.cpp: combine launches so far, one per batch of a split launch
extern "C" long hist_stub_reduces(void);    // reduce launches so far, one per batch of rows of a pair histogram

static void set_env(const char* split, const char* scratch_mb) {
  if (split) setenv("NBODY_HIST_SPLIT", split, 1); else unsetenv("NBODY_HIST_SPLIT");
  if (scratch_mb) setenv("NBODY_HIST_SCRATCH_MB", scratch_mb, 1); else unsetenv("NBODY_HIST_SCRATCH_MB");
}

static int rows(int f, int n, const float* e, int b, int* c) { return nbody_radial_counts_rows(f, n, e, b, c); }
static int rows(int f, int n, const double* e, int b, int* c) { return nbody_radial_counts_rows_d(f, n, e, b, c); }
static int at(const float* p, int m, const int* sk, const float* e, int b, int* c) { return nbody_radial_counts(p, m, sk, e, b, c); }
static int at(const double* p, int m, const int* sk, const double* e, int b, int* c) { return nbody_radial_counts_d(p, m, sk, e, b, c); }
static int pair(const float* e, int b, long long* out) { return nbody_pair_histogram(e, b, out); }
static int pair(const double* e, int b, long long* out) { return nbody_pair_histogram_d(e, b, out); }
static int nearest(const float* p, int m, const int* sk, int* i, float* d) { return nbody_nearest(p, m, sk, i, d, 0.f, nullptr); }
static int nearest(const double* p, int m, const int* sk, int* i, double* d) { return nbody_nearest_d(p, m, sk, i, d, 0.0, nullptr); }

// small integers everywhere: every value of hist_stub.cpp is exact in either precision
template <typename T>
struct Case {
  int n, m;
  std::vector<T> pos, vel, pts;
  std::vector<int> skip, counts;
  Case(int n_, int m_) : n(n_), m(m_), pos((size_t)n_ * 4), vel((size_t)n_ * 4, (T)0), pts((size_t)m_ * 4), skip((size_t)m_),
                         counts((size_t)std::max(n_, m_) * NBODY_HIST_MAX_BINS + 1) {
    for (int j = 0; j < n; ++j) { pos[4 * (size_t)j] = (T)((j * 37) % 101); pos[4 * (size_t)j + 1] = (T)(j % 7); pos[4 * (size_t)j + 2] = (T)1; pos[4 * (size_t)j + 3] = (T)(j % 977); }
    for (int p = 0; p < m; ++p) {
      pts[4 * (size_t)p] = (T)(p % 17); pts[4 * (size_t)p + 1] = (T)(p % 5); pts[4 * (size_t)p + 2] = (T)3; pts[4 * (size_t)p + 3] = (T)p;
      skip[(size_t)p] = p % 3 == 0 ? -1 : (int)(((long long)p * 7919) % n);
    }
  }
  void open(int ngpus) { OK(nbody_init(n, ngpus, sizeof(T) == 8, 0)); OK(upload<T>(pos, vel)); }
  // n_bins + 1 integer edges from 0 to 104, past every |x_j - x| (x in [0, 101)); the last one +inf when asked
  static std::vector<T> edges(int nb, bool open_end = false) {
    std::vector<T> e((size_t)nb + 1);
    for (int i = 0; i <= nb; ++i) e[(size_t)i] = (T)((104 * i + nb - 1) / nb);
    if (open_end) e[(size_t)nb] = (T)INFINITY;
    return e;
  }
  // what hist_stub.cpp makes of a query {x, w} with the excluded body sk: n_bins counts
  void expect(T x, T w, int sk, const std::vector<T>& e, int* bins) const {
    const int nb = (int)e.size() - 1;
    int cum[NBODY_HIST_MAX_BINS + 1] = {0};
    for (int b = 0; b * 1024 < n; ++b) {
      const int b0 = b * 1024, len = std::min(1024, n - b0), j = b0 + ((int)w + b) % len;
      const T d = pos[4 * (size_t)j] - x, v = d < 0 ? -d : d;
      if (j == sk) continue;
      for (int s = 0; s <= nb; ++s) cum[s] += v < e[(size_t)s];
    }
    for (int s = 0; s < nb; ++s) bins[s] = cum[s + 1] - cum[s];
  }
  void verify(int cnt_q, const std::vector<T>& e, const std::function<void(int, T*, T*, int*)>& query) {
    const int nb = (int)e.size() - 1;
    for (int q = 0; q < cnt_q; ++q) {
      T x, w; int sk, bins[NBODY_HIST_MAX_BINS];
      query(q, &x, &w, &sk);
      expect(x, w, sk, e, bins);
      for (int b = 0; b < nb; ++b) CHECK(counts[(size_t)q * nb + b] == bins[b]);
    }
    for (size_t k = (size_t)cnt_q * nb; k < counts.size(); ++k) CHECK(counts[k] == -77);   // nothing beyond
  }
  void mark() { std::fill(counts.begin(), counts.end(), -77); }
  void run_rows(int first, int count, const std::vector<T>& e) {
    mark();
    OK(rows(first, count, e.data(), (int)e.size() - 1, counts.data()));
    verify(count, e, [&](int q, T* x, T* w, int* sk) { *x = pos[4 * (size_t)(first + q)]; *w = pos[4 * (size_t)(first + q) + 3]; *sk = first + q; });
  }
  void run_points(bool with_skip, const std::vector<T>& e, int p0 = 0, int count = -1) {
    if (count < 0) count = m - p0;
    mark();
    OK(at(pts.data() + 4 * (size_t)p0, count, with_skip ? skip.data() + p0 : nullptr, e.data(), (int)e.size() - 1, counts.data()));
    verify(count, e, [&](int q, T* x, T* w, int* sk) { *x = pts[4 * (size_t)(p0 + q)]; *w = pts[4 * (size_t)(p0 + q) + 3]; *sk = with_skip ? skip[(size_t)(p0 + q)] : -1; });
  }
  // the sums of the stub's rows over all N rows, halved as the library halves them; the slots beyond n_bins stay as they were
  void run_pairs(const std::vector<T>& e) {
    const int nb = (int)e.size() - 1;
    long long got[NBODY_HIST_MAX_BINS + 1], want[NBODY_HIST_MAX_BINS] = {0};
    std::fill(got, got + NBODY_HIST_MAX_BINS + 1, -77ll);
    OK(pair(e.data(), nb, got));
    for (int i = 0; i < n; ++i) {
      int bins[NBODY_HIST_MAX_BINS];
      expect(pos[4 * (size_t)i], pos[4 * (size_t)i + 3], i, e, bins);
      for (int b = 0; b < nb; ++b) want[b] += bins[b];
    }
    for (int b = 0; b < nb; ++b) CHECK(got[b] == want[b] / 2);
    for (int b = nb; b <= NBODY_HIST_MAX_BINS; ++b) CHECK(got[b] == -77);
  }
  // nbody_nearest at the first `count` points: the nearest of the bodies the stubs offer (neighbors_stub.cpp offers the same ones)
  void run_nearest(int count) {
    std::vector<int> ni((size_t)count + 1, -77);
    std::vector<T> nd((size_t)count + 1, (T)-77);
    OK(nearest(pts.data(), count, skip.data(), ni.data(), nd.data()));
    for (int q = 0; q < count; ++q) {
      int e_idx = -1; T e_d2 = (T)INFINITY;
      const T x = pts[4 * (size_t)q], w = pts[4 * (size_t)q + 3];
      for (int b = 0; b * 1024 < n; ++b) {
        const int b0 = b * 1024, len = std::min(1024, n - b0), j = b0 + ((int)w + b) % len;
        const T d = pos[4 * (size_t)j] - x, v = d < 0 ? -d : d;
        if (j != skip[(size_t)q] && v < e_d2) { e_d2 = v; e_idx = j; }
      }
      CHECK(ni[(size_t)q] == e_idx && nd[(size_t)q] == e_d2);
    }
    CHECK(ni[(size_t)count] == -77 && nd[(size_t)count] == (T)-77);
  }
  void run_all(bool pairs = true) {
    for (int nb : {1, 5, 32}) {
      const std::vector<T> e = edges(nb), open_end = edges(nb, true);
      run_points(false, e);
      run_points(true, e);
      run_points(true, open_end);
      if (m > 2) run_points(true, e, 1, m - 2);
      const int rc = std::min(m, n);   // the row counts are the point counts, as far as there are rows
      run_rows(0, rc, e);
      run_rows(n - rc, rc, open_end);
      run_rows((n - rc) / 2, rc, e);   // a window in the middle: across the devices when there are three
      run_rows(n - 1, 1, e);
      if (pairs) { run_pairs(e); run_pairs(open_end); }
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
      c.run_all(m == 257);   // the pair histogram does not depend on m: once per n and split
    }
    set_env(nullptr, nullptr);
    SHUTDOWN();
  }
}

// The neighbour pass between histogram calls on one context: both keep their points, skip indices and split scratch in the Local's
// q_* buffers (query_pass.hpp), so each call meets buffers the other pass sized.  N = 2100: three blocks.  m = 700, n_bins = 5 over
// three chunks against 0.02 MB = 20971 B of scratch: 3 x 5 x 4 = 60 B a query, 349 fit.  One device: batches of 256 + 256 + 188.  Three
// devices: 233 or 234 queries each, fewer than one workgroup's 256, so each device's queries go as one split batch.  The count of
// combine launches (one per split batch) says that the split and the batches happened.
template <typename T>
static void interleaved(int ngpus) {
  unsetenv("NBODY_NEIGHBORS_SPLIT"); unsetenv("NBODY_NEIGHBORS_SCRATCH_MB"); unsetenv("NBODY_NEIGHBORS_LOOP");
  Case<T> c(2100, 5000);
  c.open(ngpus);
  const long batches = 3;
  for (int round = 0; round < 2; ++round) {
    set_env("3", "0.02");
    const long before = hist_stub_combines();
    c.run_points(true, Case<T>::edges(5), 0, 700);
    CHECK(hist_stub_combines() - before == batches);
    set_env(nullptr, nullptr);
    c.run_nearest(257);
    c.run_points(true, Case<T>::edges(32));
    c.run_nearest(5000);
    c.run_pairs(Case<T>::edges(5));
    c.run_points(true, Case<T>::edges(1));
  }
  SHUTDOWN();
}

int main() {
  const bool three_devices = getenv("STUB_DEVICES") && atoi(getenv("STUB_DEVICES")) >= 3;
  unsetenv("NBODY_HIST_LOOP");
  {
    float one[4] = {0, 0, 0, 0}, e[2] = {0, 1};
    double oned[4] = {0, 0, 0, 0}, ed[2] = {0, 1};
    int c[2] = {5, 5};
    long long pr[2] = {5, 5};
    CHECK(nbody_radial_counts_rows(0, 1, e, 1, c) == NBODY_ERR_NOT_INIT && nbody_radial_counts_rows_d(0, 1, ed, 1, c) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_radial_counts(one, 1, nullptr, e, 1, c) == NBODY_ERR_NOT_INIT && nbody_radial_counts_d(oned, 1, nullptr, ed, 1, c) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_pair_histogram(e, 1, pr) == NBODY_ERR_NOT_INIT && nbody_pair_histogram_d(ed, 1, pr) == NBODY_ERR_NOT_INIT);
    CHECK(c[0] == 5 && c[1] == 5 && pr[0] == 5 && pr[1] == 5);
  }

  // ---- one block, six blocks with a short last one; one device and three with ragged slices (5200 = 1733 + 1733 + 1734, 1000 = 333 + 333 + 334) ----
  for (int n : {1, 1000, 5200}) {
    shapes<float>(n, 1);
    if (three_devices && n >= 3) shapes<float>(n, 3);
  }
  shapes<double>(5200, 1);
  if (three_devices) shapes<double>(1000, 3);

  // ---- the batched path: 5000 queries x 6 chunks x n_bins x 4 B against 0.05 MB = 52428 B: n_bins = 1 (24 B a query) in batches of
  //      2048, n_bins = 5 (120 B: 436 fit) in batches of 256, n_bins = 32 (768 B: 68 fit) not one workgroup, hence unsplit; against 1 MB:
  //      n_bins = 32 in batches of 1280.  The pair histogram's rows: 0.05 MB holds 13107, 2621 and 409 rows of 1, 5 and 32 bins: batches
  //      of 13056 (all 5200 rows at once), 2560 and 256 ----
  for (int ngpus : {1, 3}) {
    if (ngpus > 1 && !three_devices) continue;
    Case<float> c(5200, 5000);
    c.open(ngpus);
    for (const char* mb : {"0.05", "1"})
      for (const char* split : {(const char*)nullptr, "4", "6"}) {
        set_env(split, mb);
        const long before = hist_stub_combines();
        c.run_all();
        CHECK(hist_stub_combines() > before);
      }
    set_env(nullptr, "0.05");
    long before = hist_stub_reduces();
    c.run_pairs(Case<float>::edges(32));
    CHECK(hist_stub_reduces() - before == 21);   // 5200 rows = 20 x 256 + 80; 1733, 1733, 1734 rows = 3 x 7 batches
    set_env(nullptr, "0");    // not one workgroup's queries fit: no split; the pair histogram's rows go 256 at a time
    before = hist_stub_combines();
    c.run_all();
    set_env("5", "0");
    c.run_all();
    CHECK(hist_stub_combines() == before);
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
    int* K = c.counts.data();
    std::vector<float> e = Case<float>::edges(5);
    long long pr[NBODY_HIST_MAX_BINS];
    std::fill(pr, pr + NBODY_HIST_MAX_BINS, -77ll);
    CHECK(nbody_radial_counts_rows(0, 300, e.data(), 5, nullptr) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts_rows(0, 300, nullptr, 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts(pts, 300, nullptr, e.data(), 5, nullptr) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts(pts, 300, nullptr, nullptr, 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts(nullptr, 300, nullptr, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_pair_histogram(e.data(), 5, nullptr) == NBODY_ERR_ARG);
    CHECK(nbody_pair_histogram(nullptr, 5, pr) == NBODY_ERR_ARG);
    for (int nb : {0, -1, NBODY_HIST_MAX_BINS + 1, 1 << 30}) {
      CHECK(nbody_radial_counts_rows(0, 300, e.data(), nb, K) == NBODY_ERR_ARG);
      CHECK(nbody_radial_counts(pts, 300, nullptr, e.data(), nb, K) == NBODY_ERR_ARG);
      CHECK(nbody_pair_histogram(e.data(), nb, pr) == NBODY_ERR_ARG);
    }
    for (int at_ : {0, 3, 5})
      for (float bad : {NAN, -1.0f}) {   // a NaN edge; an edge below the one before it (-1 at slot 0 is legal: skipped)
        std::vector<float> b = e;
        if (bad < 0 && at_ == 0) continue;
        b[(size_t)at_] = bad;
        CHECK(nbody_radial_counts_rows(0, 300, b.data(), 5, K) == NBODY_ERR_ARG);
        CHECK(nbody_radial_counts(pts, 300, nullptr, b.data(), 5, K) == NBODY_ERR_ARG);
        CHECK(nbody_pair_histogram(b.data(), 5, pr) == NBODY_ERR_ARG);
      }
    CHECK(nbody_radial_counts_rows(-1, 300, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts_rows(0, 0, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts_rows(0, -4, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts_rows(5200, 1, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts_rows(5000, 201, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts_rows(1 << 30, 1 << 30, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts(pts, 0, nullptr, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts(pts, -1, nullptr, e.data(), 5, K) == NBODY_ERR_ARG);
    for (int bad : {5200, -2, 1 << 30}) {
      std::vector<int> sk = c.skip;
      sk[299] = bad;
      CHECK(nbody_radial_counts(pts, 300, sk.data(), e.data(), 5, K) == NBODY_ERR_ARG);
    }
    std::vector<double> pd(1200, 0.0), ed = Case<double>::edges(5);
    CHECK(nbody_radial_counts_d(pd.data(), 300, nullptr, ed.data(), 5, K) == NBODY_ERR_STATE);
    CHECK(nbody_radial_counts_rows_d(0, 300, ed.data(), 5, K) == NBODY_ERR_STATE);
    CHECK(nbody_pair_histogram_d(ed.data(), 5, pr) == NBODY_ERR_STATE);
    for (size_t k = 0; k < c.counts.size(); ++k) CHECK(c.counts[k] == -77);
    for (int b = 0; b < NBODY_HIST_MAX_BINS; ++b) CHECK(pr[b] == -77);
    std::vector<int> edge = c.skip;
    edge[0] = 5199; edge[299] = 0;
    OK(nbody_radial_counts(pts, 300, edge.data(), e.data(), 5, K));
    CHECK(c.counts[0] != -77 && c.counts[300 * 5] == -77);
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_radial_counts(pts, 10, nullptr, e.data(), 5, K) == NBODY_ERR_STATE && nbody_radial_counts_rows(0, 10, e.data(), 5, K) == NBODY_ERR_STATE);
    CHECK(nbody_pair_histogram(e.data(), 5, pr) == NBODY_ERR_STATE);
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
    const std::vector<float> e5 = Case<float>::edges(5), e32 = Case<float>::edges(32), e1 = Case<float>::edges(1);
    set_env("3", nullptr);
    int made = sweep("nbody_radial_counts split", [&] { c.open(ngpus); },
                     [&] { return nbody_radial_counts(c.pts.data(), c.m, c.skip.data(), e5.data(), 5, c.counts.data()); }, [&] { c.run_points(true, e5); });
    CHECK(made == 4 * ngpus);   // points, skip, counts, scratch per device
    made = sweep("nbody_radial_counts_rows split", [&] { c.open(ngpus); }, [&] { return nbody_radial_counts_rows(0, 5200, e32.data(), 32, c.counts.data()); },
                 [&] { c.run_rows(0, 5200, e32); });
    CHECK(made == 2 * ngpus);   // counts, scratch
    long long pr[NBODY_HIST_MAX_BINS];
    made = sweep("nbody_pair_histogram split", [&] { c.open(ngpus); }, [&] { return nbody_pair_histogram(e5.data(), 5, pr); }, [&] { c.run_pairs(e5); });
    CHECK(made == 3 * ngpus);   // sums, counts, scratch
    set_env("1", nullptr);
    made = sweep("nbody_radial_counts", [&] { c.open(ngpus); }, [&] { return nbody_radial_counts(c.pts.data(), c.m, nullptr, e1.data(), 1, c.counts.data()); },
                 [&] { c.run_points(false, e1); });
    CHECK(made == 2 * ngpus);   // points, counts
  }
  set_env(nullptr, nullptr);
  printf("hist_sanity ok\n");
  return 0;
}
