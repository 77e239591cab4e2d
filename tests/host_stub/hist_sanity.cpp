// hist_sanity.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py, case `hist`): drives nbody_radial_counts_rows, nbody_radial_counts and
// nbody_pair_histogram (and their _d forms) of the library's host code (hist.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp,
// neighbors.cpp) against tests/host_stub/hip_stub.cpp and hist_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's
// logic: the edge slots, the rows of a window and the division of the points over the devices, the upload and copy-back offsets of
// [m][n_bins] outputs, the choice of the source split, the n_bins-dependent scratch size and the batches, the batches of rows of the
// pair histogram and the sum over the devices, the argument checks, lifetimes at shutdown and the failure paths.  hist_stub.cpp states
// the values expected here.  neighbors_stub.cpp is linked for neighbors.cpp; nbody_nearest runs between histogram calls on one context
// (the passes share their query buffers).  It covers one and three stub devices with ragged slices, n_bins 1, 5 and 32, m = 1, 255,
// 256, 257 and 5000, the source split forced and automatic, the batched path of the queries and of the pair histogram's rows, every
// NBODY_ERR_ARG case and the failure sweep of sanity_common.hpp.
#include <math.h>
#include <string.h>

#define SANITY_NAME "hist_sanity"
#include "sanity_common.hpp"

extern "C" long hist_stub_combines(void);   // hist_stub.cpp: combine launches so far, one per batch of a split launch
extern "C" long hist_stub_reduces(void);    // reduce launches so far, one per batch of rows of a pair histogram

static const SplitEnv env = {"NBODY_HIST_SPLIT", "NBODY_HIST_SCRATCH_MB"};

static int rows(int f, int n, const float* e, int b, int* c) { return nbody_radial_counts_rows(f, n, e, b, c); }
static int rows(int f, int n, const double* e, int b, int* c) { return nbody_radial_counts_rows_d(f, n, e, b, c); }
static int at(const float* p, int m, const int* sk, const float* e, int b, int* c) { return nbody_radial_counts(p, m, sk, e, b, c); }
static int at(const double* p, int m, const int* sk, const double* e, int b, int* c) { return nbody_radial_counts_d(p, m, sk, e, b, c); }
static int pair(const float* e, int b, long long* out) { return nbody_pair_histogram(e, b, out); }
static int pair(const double* e, int b, long long* out) { return nbody_pair_histogram_d(e, b, out); }
static int nearest(const float* p, int m, const int* sk, int* i, float* d) { return nbody_nearest(p, m, sk, i, d, 0.f, nullptr); }
static int nearest(const double* p, int m, const int* sk, int* i, double* d) { return nbody_nearest_d(p, m, sk, i, d, 0.0, nullptr); }

template <typename T>
struct Case : Fixture<T> {
  using F = Fixture<T>;
  using Q = typename F::Q;
  using F::n; using F::m; using F::pos; using F::pts; using F::skip;
  std::vector<int> counts;
  Case(int n_, int m_) : F(n_, m_), counts((size_t)std::max(n_, m_) * NBODY_HIST_MAX_BINS + 1) {}
  // n_bins + 1 integer edges from 0 to 104, past every |x_j - x| (x in [0, 101)); the last one +inf when asked
  static std::vector<T> edges(int nb, bool open_end = false) {
    std::vector<T> e((size_t)nb + 1);
    for (int i = 0; i <= nb; ++i) e[(size_t)i] = (T)((104 * i + nb - 1) / nb);
    if (open_end) e[(size_t)nb] = (T)INFINITY;
    return e;
  }
  // what hist_stub.cpp makes of a query: n_bins counts
  void expect(const Q& q, const std::vector<T>& e, int* bins) const {
    const int nb = (int)e.size() - 1;
    int cum[NBODY_HIST_MAX_BINS + 1] = {0};
    for (int b = 0; b < stub::blocks_of(n); ++b) {
      const int j = stub::candidate(n, q.w, b).j;
      if (j == q.sk) continue;
      const T v = stub::absdiff(pos[4 * (size_t)j], q.x);
      for (int s = 0; s <= nb; ++s) cum[s] += v < e[(size_t)s];
    }
    for (int s = 0; s < nb; ++s) bins[s] = cum[s + 1] - cum[s];
  }
  void verify(int cnt_q, const std::vector<T>& e, const std::function<Q(int)>& query) {
    const int nb = (int)e.size() - 1;
    for (int q = 0; q < cnt_q; ++q) {
      int bins[NBODY_HIST_MAX_BINS];
      expect(query(q), e, bins);
      for (int b = 0; b < nb; ++b) CHECK(counts[(size_t)q * nb + b] == bins[b]);
    }
    CHECK(nothing_beyond(counts, (size_t)cnt_q * nb));
  }
  void run_rows(int first, int count, const std::vector<T>& e) {
    mark(counts);
    OK(rows(first, count, e.data(), (int)e.size() - 1, counts.data()));
    verify(count, e, [&](int q) { return this->row(first + q); });
  }
  void run_points(bool with_skip, const std::vector<T>& e, int p0 = 0, int count = -1) {
    if (count < 0) count = m - p0;
    mark(counts);
    OK(at(pts.data() + 4 * (size_t)p0, count, with_skip ? skip.data() + p0 : nullptr, e.data(), (int)e.size() - 1, counts.data()));
    verify(count, e, [&](int q) { return this->point(p0 + q, with_skip); });
  }
  // the sums of the stub's rows over all N rows, halved as the library halves them; the slots beyond n_bins stay as they were
  void run_pairs(const std::vector<T>& e) {
    const int nb = (int)e.size() - 1;
    long long got[NBODY_HIST_MAX_BINS + 1], want[NBODY_HIST_MAX_BINS] = {0};
    std::fill(got, got + NBODY_HIST_MAX_BINS + 1, (long long)kMark);
    OK(pair(e.data(), nb, got));
    for (int i = 0; i < n; ++i) {
      int bins[NBODY_HIST_MAX_BINS];
      expect(this->row(i), e, bins);
      for (int b = 0; b < nb; ++b) want[b] += bins[b];
    }
    for (int b = 0; b < nb; ++b) CHECK(got[b] == want[b] / 2);
    for (int b = nb; b <= NBODY_HIST_MAX_BINS; ++b) CHECK(got[b] == kMark);
  }
  // nbody_nearest at the first `count` points: the nearest of the bodies the stubs offer (neighbors_stub.cpp offers the same ones)
  void run_nearest(int count) {
    std::vector<int> ni((size_t)count + 1, kMark);
    std::vector<T> nd((size_t)count + 1, (T)kMark);
    OK(nearest(pts.data(), count, skip.data(), ni.data(), nd.data()));
    for (int p = 0; p < count; ++p) {
      int e_idx = -1; T e_d2 = (T)INFINITY;
      const Q q = this->point(p, true);
      for (int b = 0; b < stub::blocks_of(n); ++b) {
        const int j = stub::candidate(n, q.w, b).j;
        const T v = stub::absdiff(pos[4 * (size_t)j], q.x);
        if (j != q.sk && v < e_d2) { e_d2 = v; e_idx = j; }
      }
      CHECK(ni[(size_t)p] == e_idx && nd[(size_t)p] == e_d2);
    }
    CHECK(nothing_beyond(ni, (size_t)count) && nothing_beyond(nd, (size_t)count));
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
  for (int m : kShapeM) {
    Case<T> c(n, m);
    c.open(ngpus);
    for_splits(env, {nullptr, "0", "1", "3", "1000"}, [&] { c.run_all(m == 257); });   // the pair histogram does not depend on m: once per n and split
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
    env.set("3", "0.02");
    const long before = hist_stub_combines();
    c.run_points(true, Case<T>::edges(5), 0, 700);
    CHECK(hist_stub_combines() - before == batches);
    env.set(nullptr, nullptr);
    c.run_nearest(257);
    c.run_points(true, Case<T>::edges(32));
    c.run_nearest(5000);
    c.run_pairs(Case<T>::edges(5));
    c.run_points(true, Case<T>::edges(1));
  }
  SHUTDOWN();
}

int main() {
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
  for_sizes({1, 1000, 5200}, shapes<float>, shapes<double>);

  // ---- the batched path: 5000 queries x 6 chunks x n_bins x 4 B against 0.05 MB = 52428 B: n_bins = 1 (24 B a query) in batches of
  //      2048, n_bins = 5 (120 B: 436 fit) in batches of 256, n_bins = 32 (768 B: 68 fit) not one workgroup, hence unsplit; against 1 MB:
  //      n_bins = 32 in batches of 1280.  The pair histogram's rows: 0.05 MB holds 13107, 2621 and 409 rows of 1, 5 and 32 bins: batches
  //      of 13056 (all 5200 rows at once), 2560 and 256 ----
  for_device_counts([](int ngpus) {
    Case<float> c(5200, 5000);
    c.open(ngpus);
    for (const char* mb : {"0.05", "1"})
      for (const char* split : {(const char*)nullptr, "4", "6"}) {
        env.set(split, mb);
        const long before = hist_stub_combines();
        c.run_all();
        CHECK(hist_stub_combines() > before);
      }
    env.set(nullptr, "0.05");
    long before = hist_stub_reduces();
    c.run_pairs(Case<float>::edges(32));
    CHECK(hist_stub_reduces() - before == 21);   // 5200 rows = 20 x 256 + 80; 1733, 1733, 1734 rows = 3 x 7 batches
    env.set(nullptr, "0");    // not one workgroup's queries fit: no split; the pair histogram's rows go 256 at a time
    before = hist_stub_combines();
    c.run_all();
    env.set("5", "0");
    c.run_all();
    CHECK(hist_stub_combines() == before);
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
    mark(c.counts);
    int* K = c.counts.data();
    std::vector<float> e = Case<float>::edges(5);
    long long pr[NBODY_HIST_MAX_BINS];
    std::fill(pr, pr + NBODY_HIST_MAX_BINS, (long long)kMark);
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
    for (const Window& w : refused_windows(5200, 300)) CHECK(nbody_radial_counts_rows(w.first, w.count, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts(pts, 0, nullptr, e.data(), 5, K) == NBODY_ERR_ARG);
    CHECK(nbody_radial_counts(pts, -1, nullptr, e.data(), 5, K) == NBODY_ERR_ARG);
    for (int bad : refused_skips(5200)) CHECK(nbody_radial_counts(pts, 300, c.skip_with(299, bad).data(), e.data(), 5, K) == NBODY_ERR_ARG);
    std::vector<double> pd(1200, 0.0), ed = Case<double>::edges(5);
    CHECK(nbody_radial_counts_d(pd.data(), 300, nullptr, ed.data(), 5, K) == NBODY_ERR_STATE);
    CHECK(nbody_radial_counts_rows_d(0, 300, ed.data(), 5, K) == NBODY_ERR_STATE);
    CHECK(nbody_pair_histogram_d(ed.data(), 5, pr) == NBODY_ERR_STATE);
    CHECK(nothing_beyond(c.counts, 0));
    for (int b = 0; b < NBODY_HIST_MAX_BINS; ++b) CHECK(pr[b] == kMark);
    std::vector<int> edge = c.skip;
    edge[0] = 5199; edge[299] = 0;
    OK(nbody_radial_counts(pts, 300, edge.data(), e.data(), 5, K));
    CHECK(c.counts[0] != kMark && c.counts[300 * 5] == kMark);
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
  for_device_counts([](int ngpus) {
    interleaved<float>(ngpus);
    interleaved<double>(ngpus);
  });

  // ---- the failure paths: every allocating call of a call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(5200, 700);
    const std::vector<float> e5 = Case<float>::edges(5), e32 = Case<float>::edges(32), e1 = Case<float>::edges(1);
    env.set("3", nullptr);
    int made = sweep("nbody_radial_counts split", [&] { c.open(ngpus); },
                     [&] { return nbody_radial_counts(c.pts.data(), c.m, c.skip.data(), e5.data(), 5, c.counts.data()); }, [&] { c.run_points(true, e5); });
    CHECK(made == 4 * ngpus);   // points, skip, counts, scratch per device
    made = sweep("nbody_radial_counts_rows split", [&] { c.open(ngpus); }, [&] { return nbody_radial_counts_rows(0, 5200, e32.data(), 32, c.counts.data()); },
                 [&] { c.run_rows(0, 5200, e32); });
    CHECK(made == 2 * ngpus);   // counts, scratch
    long long pr[NBODY_HIST_MAX_BINS];
    made = sweep("nbody_pair_histogram split", [&] { c.open(ngpus); }, [&] { return nbody_pair_histogram(e5.data(), 5, pr); }, [&] { c.run_pairs(e5); });
    CHECK(made == 3 * ngpus);   // sums, counts, scratch
    env.set("1", nullptr);
    made = sweep("nbody_radial_counts", [&] { c.open(ngpus); }, [&] { return nbody_radial_counts(c.pts.data(), c.m, nullptr, e1.data(), 1, c.counts.data()); },
                 [&] { c.run_points(false, e1); });
    CHECK(made == 2 * ngpus);   // points, counts
  });
  env.set(nullptr, nullptr);
  printf("hist_sanity ok\n");
  return 0;
}
