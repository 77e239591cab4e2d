// fof_sanity.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): drives nbody_fof and nbody_fof_d of the library's host
// code (fof.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp, point_sums.cpp, neighbors.cpp, knn.cpp) against
// tests/host_stub/hip_stub.cpp and fof_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's logic: the union-find and
// its rounds, the division of the active rows over the devices, the upload of the labels and of the active-row list, the copy-back
// offsets, the choice of the source split, the scratch size and the batches, the argument checks, lifetimes at shutdown and the
// failure paths.  The system is one-dimensional — body j at x = s + 2 (s / 7) with s = 7919 j mod N, a bijection, so that along the
// line every seventh gap is 3 and the others 1 while neighbours on the line are far apart in index — and its groups are found here by
// sorting: b2 = 0 links nothing, b2 = 1 the runs of seven, b2 = 9 everything.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <numeric>

#define SANITY_NAME "fof_sanity"
#include "sanity_common.hpp"

extern "C" long fof_stub_combines(void);   // fof_stub.cpp: combine launches so far, one per batch of a split launch
extern "C" long fof_stub_rows(void);       // rows walked so far
extern "C" long fof_stub_listed(void);     // ... of which from an active-row list

static const SplitEnv env = {"NBODY_FOF_SPLIT", "NBODY_FOF_SCRATCH_MB"};
// the pass's third variable beside them: every row in every round
static void fof_env(const char* split, const char* scratch_mb, const char* all_rows = nullptr) {
  env.set(split, scratch_mb);
  set_env("NBODY_FOF_ALL_ROWS", all_rows);
}

static int fof(float b2, int* g, int* ng, int* r) { return nbody_fof(b2, g, ng, r); }
static int fof(double b2, int* g, int* ng, int* r) { return nbody_fof_d(b2, g, ng, r); }

static int round_cap(int n) {
  int cap = 1;
  for (long long p = 1; p < n; p *= 2) ++cap;
  return cap;
}

template <typename T>
struct Case : System<T> {
  using System<T>::n; using System<T>::pos;
  std::vector<int> group, want;
  explicit Case(int n_) : System<T>(n_), group((size_t)n_ + 1), want((size_t)n_) {
    for (int j = 0; j < n; ++j) {
      const int s = (int)(((long long)j * 7919) % n);
      this->set(pos, j, (T)(s + 2 * (s / 7)), (T)1, (T)2, (T)1);
    }
  }
  // the groups at b2 by sorting along the line; returns their number
  int expect(T b2) {
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return pos[4 * (size_t)a] < pos[4 * (size_t)b]; });
    int groups = 0;
    for (int a = 0; a < n;) {
      int b = a + 1, low = order[(size_t)a];
      for (; b < n; ++b) {
        const T d = pos[4 * (size_t)order[(size_t)b]] - pos[4 * (size_t)order[(size_t)b - 1]];
        if (!(d * d <= b2)) break;
        low = std::min(low, order[(size_t)b]);
      }
      for (int k = a; k < b; ++k) want[(size_t)order[(size_t)k]] = low;
      ++groups;
      a = b;
    }
    return groups;
  }
  // one call with the outputs asked for; returns the rounds (kMark when not asked for)
  int run(T b2, bool w_group = true, bool w_count = true, bool w_rounds = true) {
    const int groups = expect(b2);
    mark(group);
    int ng = kMark, rounds = kMark;
    OK(fof(b2, w_group ? group.data() : nullptr, w_count ? &ng : nullptr, w_rounds ? &rounds : nullptr));
    for (int i = 0; i < n; ++i) CHECK(group[(size_t)i] == (w_group ? want[(size_t)i] : kMark));
    CHECK(nothing_beyond(group, (size_t)n));
    CHECK(ng == (w_count ? groups : kMark));
    CHECK(w_rounds ? rounds >= 1 && rounds <= round_cap(n) : rounds == kMark);
    return rounds;
  }
  void run_all() {
    for (T b2 : {(T)0, (T)1, (T)9, (T)INFINITY}) {
      if (b2 > (T)9 && n > 1000) continue;   // (+inf gives what 9 gives; once per size class is enough)
      fof_env(nullptr, nullptr);
      const long listed0 = fof_stub_listed(), rows0 = fof_stub_rows();
      const int rounds = run(b2);
      const long listed = fof_stub_listed() - listed0, walked = fof_stub_rows() - rows0;
      CHECK(b2 == (T)0 || n == 1 ? rounds == 1 : rounds >= 2);
      CHECK((listed > 0) == (rounds >= 2));   // every round but the first walks a list of the rows of the groups that reported
      CHECK(walked <= (long)rounds * n);
      CHECK(run(b2, true, false, true) == rounds);
      CHECK(run(b2, false, true, true) == rounds);
      run(b2, true, true, false);
      for (const char* split : {"0", "1", "3", "1000"}) {
        fof_env(split, nullptr);
        CHECK(run(b2) == rounds);
      }
      fof_env(nullptr, nullptr, "1");   // every row in every round: the same groups, the same rounds, no list
      const long l1 = fof_stub_listed(), r1 = fof_stub_rows();
      CHECK(run(b2) == rounds);
      CHECK(fof_stub_listed() == l1 && fof_stub_rows() - r1 == (long)rounds * n && walked <= (long)rounds * n);
      fof_env("2", nullptr, "1");
      CHECK(run(b2) == rounds);
    }
    fof_env(nullptr, nullptr);
  }
};

template <typename T>
static void shapes(int n, int ngpus) {
  Case<T> c(n);
  c.open(ngpus);
  c.run_all();
  SHUTDOWN();
}

int main() {
  {
    int gr[2] = {5, 5}, ng = 5, r = 5;
    CHECK(nbody_fof(1.f, gr, &ng, &r) == NBODY_ERR_NOT_INIT && nbody_fof_d(1.0, gr, &ng, &r) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_fof(-1.f, nullptr, nullptr, nullptr) == NBODY_ERR_NOT_INIT);
    CHECK(gr[0] == 5 && gr[1] == 5 && ng == 5 && r == 5);
  }

  // ---- one block, five blocks with a short last one; one device and three with ragged ranges ----
  for (int n : {1, 255, 256, 257, 5000}) {
    shapes<float>(n, 1);
    if (three_devices() && n >= 3) shapes<float>(n, 3);
  }
  shapes<double>(257, 1);
  if (three_devices()) shapes<double>(5000, 3);

  // ---- the batched path: 5000 rows x 5 chunks x 4 B = 100 kB against 0.01 MB = 10485 B: 524 rows fit, batches of 512; three devices:
  //      1666 or 1667 rows each, batches of 512 likewise.  Against 0: not one workgroup's rows fit, hence unsplit ----
  for_device_counts([](int ngpus) {
    Case<float> c(5000);
    c.open(ngpus);
    fof_env(nullptr, nullptr);
    const int rounds = c.run(1.f);
    for (const char* split : {"5", "2"}) {
      fof_env(split, "0.01");
      const long before = fof_stub_combines();
      CHECK(c.run(1.f) == rounds);
      // five chunks, the first round alone: ceil(5000 / 512) or 3 x ceil(1667 / 512) batches; two chunks: 1310 rows fit, batches of 1280
      CHECK(fof_stub_combines() - before >= (split[0] == '2' ? 4 : ngpus == 1 ? 10 : 12));
    }
    fof_env("5", "0.01", "1");
    CHECK(c.run(9.f) == c.run(9.f));
    fof_env("5", "0");
    const long before = fof_stub_combines();
    CHECK(c.run(1.f) == rounds);
    CHECK(fof_stub_combines() == before);
    fof_env(nullptr, nullptr);
    SHUTDOWN();
  });

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(1000);
    c.open(three_devices() ? 3 : 1);
    mark(c.group);
    int ng = kMark, r = kMark;
    CHECK(nbody_fof(1.f, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    CHECK(nbody_fof(1.f, nullptr, nullptr, &r) == NBODY_ERR_ARG);
    for (float bad : {(float)NAN, -1.f, -0.5f, -(float)INFINITY, -1e-30f}) CHECK(nbody_fof(bad, c.group.data(), &ng, &r) == NBODY_ERR_ARG);
    CHECK(nbody_fof_d(1.0, c.group.data(), &ng, &r) == NBODY_ERR_STATE);
    CHECK(nothing_beyond(c.group, 0));
    CHECK(ng == kMark && r == kMark);
    c.run(-0.f);   // minus zero is zero: legal
    c.run_all();
    SHUTDOWN();
    Case<double> d(300);
    d.open(1);
    CHECK(nbody_fof(1.f, c.group.data(), &ng, &r) == NBODY_ERR_STATE);
    CHECK(nbody_fof_d((double)NAN, d.group.data(), &ng, &r) == NBODY_ERR_ARG && nbody_fof_d(-1.0, d.group.data(), &ng, &r) == NBODY_ERR_ARG);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a call, one device and three, split (scratch) and not, one round and several ----
  for_device_counts([](int ngpus) {
    Case<float> c(2100);   // three blocks
    int ng = 0, r = 0;
    fof_env("3", nullptr);
    int made = sweep("nbody_fof one round, split", [&] { c.open(ngpus); }, [&] { return nbody_fof(0.f, c.group.data(), &ng, &r); }, [&] { c.run(0.f); });
    CHECK(made == 3 * ngpus);   // labels, m, scratch per device
    made = sweep("nbody_fof rounds, split", [&] { c.open(ngpus); }, [&] { return nbody_fof(1.f, c.group.data(), &ng, &r); }, [&] { c.run(1.f); });
    CHECK(made == 4 * ngpus);   // ... and the active-row list
    fof_env("1", nullptr);
    made = sweep("nbody_fof rounds", [&] { c.open(ngpus); }, [&] { return nbody_fof(9.f, nullptr, &ng, nullptr); }, [&] { c.run(9.f, false, true, false); });
    CHECK(made == 3 * ngpus);   // labels, m, the active-row list
  });
  fof_env(nullptr, nullptr);
  printf("fof_sanity ok\n");
  return 0;
}
