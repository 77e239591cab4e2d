// field_sanity.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): drives nbody_field(_d) of the library's host code
// (field.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp) against tests/host_stub/hip_stub.cpp and field_stub.cpp under
// AddressSanitizer + UBSan.  What it checks is the host's logic: the division of the points over the devices, the upload and copy-back
// offsets, the choice of the source split, the scratch size and the batches, the argument checks, lifetimes at shutdown and the
// failure paths.  field_stub.cpp states the values expected here.
#include <string.h>

#define SANITY_NAME "field_sanity"
#include "sanity_common.hpp"

static void set_env(const char* split, const char* scratch_mb) {
  if (split) setenv("NBODY_FIELD_SPLIT", split, 1); else unsetenv("NBODY_FIELD_SPLIT");
  if (scratch_mb) setenv("NBODY_FIELD_SCRATCH_MB", scratch_mb, 1); else unsetenv("NBODY_FIELD_SCRATCH_MB");
}

static int field(const float* p, int m, const int* sk, float* a, float* phi) { return nbody_field(p, m, sk, a, phi); }
static int field(const double* p, int m, const int* sk, double* a, double* phi) { return nbody_field_d(p, m, sk, a, phi); }

// small integers everywhere: every sum of field_stub.cpp is exact in either precision
template <typename T>
struct Case {
  int n, m;
  std::vector<T> pos, vel, pts, acc, phi;
  std::vector<int> skip;
  Case(int n_, int m_) : n(n_), m(m_), pos((size_t)n_ * 4), vel((size_t)n_ * 4, (T)0), pts((size_t)m_ * 4), acc((size_t)m_ * 4), phi((size_t)m_), skip((size_t)m_) {
    for (int j = 0; j < n; ++j) { pos[4 * (size_t)j] = (T)(j % 13); pos[4 * (size_t)j + 1] = (T)(j % 7); pos[4 * (size_t)j + 2] = (T)1; pos[4 * (size_t)j + 3] = (T)1; }
    for (int p = 0; p < m; ++p) {
      pts[4 * (size_t)p] = (T)(p % 17); pts[4 * (size_t)p + 1] = (T)(p % 5); pts[4 * (size_t)p + 2] = (T)3; pts[4 * (size_t)p + 3] = (T)p;
      skip[(size_t)p] = p % 3 == 0 ? -1 : (int)(((long long)p * 7919) % n);
    }
  }
  void open(int ngpus) { OK(nbody_init(n, ngpus, sizeof(T) == 8, 0)); OK(upload<T>(pos, vel)); }
  // points [p0, p0 + cnt) of the case, with or without skip and either output
  void run(bool with_skip, bool want_acc, bool want_phi, int p0 = 0, int cnt = -1) {
    if (cnt < 0) cnt = m - p0;
    const T mark = (T)-77;
    std::fill(acc.begin(), acc.end(), mark);
    std::fill(phi.begin(), phi.end(), mark);
    OK(field(pts.data() + 4 * (size_t)p0, cnt, with_skip ? skip.data() + p0 : nullptr, want_acc ? acc.data() : nullptr, want_phi ? phi.data() : nullptr));
    const int nb = (n + 1023) / 1024;
    for (int k = 0; k < cnt; ++k) {
      const int p = p0 + k;
      double ax = 0.0, ay = 0.0;
      for (int b = 0; b < nb; ++b) { ax += (double)(T)((T)((b * 1024) % 13) - (T)(p % 17)); ay += (double)(T)((T)(p % 5) + (T)b); }
      const double az = (double)nb * (double)(with_skip ? skip[(size_t)p] : -1) + (double)((n - 1) % 13);
      if (want_acc) CHECK(acc[4 * (size_t)k] == (T)ax && acc[4 * (size_t)k + 1] == (T)ay && acc[4 * (size_t)k + 2] == (T)az && acc[4 * (size_t)k + 3] == (T)0);
      else CHECK(acc[4 * (size_t)k] == mark);
      if (want_phi) CHECK(phi[(size_t)k] == (T)(0.0 - (double)nb * (double)p));
      else CHECK(phi[(size_t)k] == mark);
    }
    for (size_t k = (size_t)cnt; k < (size_t)m; ++k) CHECK(acc[4 * k] == mark && phi[k] == mark);   // nothing beyond the points asked for
  }
  void run_all() {
    run(false, true, true);
    run(true, true, true);
    run(true, true, false);
    run(false, false, true);
    if (m > 2) run(true, true, true, 1, m - 2);
  }
};

template <typename T>
static void shapes(int n, int ngpus) {
  for (int m : {1, 255, 256, 257, 5000}) {
    Case<T> c(n, m);
    c.open(ngpus);
    for (const char* split : {(const char*)nullptr, "0", "1", "2", "3", "1000"}) {
      set_env(split, nullptr);
      c.run_all();
    }
    SHUTDOWN();
  }
  set_env(nullptr, nullptr);
}

int main() {
  const bool three_devices = getenv("STUB_DEVICES") && atoi(getenv("STUB_DEVICES")) >= 3;
  float one[4] = {0, 0, 0, 0}, out[4] = {5, 5, 5, 5}, ph[1] = {5};
  double oned[4] = {0, 0, 0, 0}, outd[4] = {5, 5, 5, 5}, phd[1] = {5};
  CHECK(nbody_field(one, 1, nullptr, out, ph) == NBODY_ERR_NOT_INIT && nbody_field_d(oned, 1, nullptr, outd, phd) == NBODY_ERR_NOT_INIT);

  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 + 695 + 695, 1000 = 333 + 333 + 334) ----
  for (int n : {1, 1000, 2085}) {
    shapes<float>(n, 1);
    if (three_devices && n >= 3) shapes<float>(n, 3);
  }
  shapes<double>(2085, 1);
  if (three_devices) shapes<double>(1000, 3);

  // ---- the batched path: 69 blocks x 16 B = 1104 B of per-block sums per point against 1 MB: batches of 768 points (fp32) ----
  for (int ngpus : {1, 3}) {
    if (ngpus > 1 && !three_devices) continue;
    Case<float> c(70000, 5000);
    c.open(ngpus);
    for (const char* split : {(const char*)nullptr, "7", "69"}) {
      set_env(split, "1");
      c.run_all();
    }
    set_env(nullptr, "0");    // not one workgroup's points fit: no split
    c.run_all();
    set_env("5", "0");
    c.run_all();
    SHUTDOWN();
  }
  {
    Case<double> c(70000, 1000);   // 2208 B per point: batches of 256
    c.open(1);
    set_env(nullptr, "1");
    c.run_all();
    SHUTDOWN();
  }
  set_env(nullptr, nullptr);

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(2085, 300);
    c.open(three_devices ? 3 : 1);
    float* pts = c.pts.data();
    std::fill(c.acc.begin(), c.acc.end(), -77.f);
    std::fill(c.phi.begin(), c.phi.end(), -77.f);
    CHECK(nbody_field(nullptr, 300, nullptr, c.acc.data(), c.phi.data()) == NBODY_ERR_ARG);
    CHECK(nbody_field(pts, 0, nullptr, c.acc.data(), c.phi.data()) == NBODY_ERR_ARG);
    CHECK(nbody_field(pts, -1, nullptr, c.acc.data(), c.phi.data()) == NBODY_ERR_ARG);
    CHECK(nbody_field(pts, 300, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    for (int bad : {2085, -2, 1 << 30}) {
      std::vector<int> sk = c.skip;
      sk[299] = bad;
      CHECK(nbody_field(pts, 300, sk.data(), c.acc.data(), c.phi.data()) == NBODY_ERR_ARG);
    }
    std::vector<int> edge = c.skip;
    edge[0] = 2084; edge[299] = 0;
    OK(nbody_field(pts, 300, edge.data(), nullptr, c.phi.data()));
    for (float v : c.acc) CHECK(v == -77.f);
    std::vector<double> pd(1200, 0.0), ad(1200, 5.0), fd(300, 5.0);
    CHECK(nbody_field_d(pd.data(), 300, nullptr, ad.data(), fd.data()) == NBODY_ERR_STATE && ad[0] == 5.0 && fd[299] == 5.0);
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_field(pts, 10, nullptr, c.acc.data(), c.phi.data()) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a field call, one device and three, split (scratch) and not ----
  for (int ngpus : {1, 3}) {
    if (ngpus > 1 && !three_devices) continue;
    Case<float> c(2085, 700);
    set_env("3", nullptr);
    int made = sweep("nbody_field split", [&] { c.open(ngpus); }, [&] { return nbody_field(c.pts.data(), c.m, c.skip.data(), c.acc.data(), c.phi.data()); },
                     [&] { c.run(true, true, true); });
    CHECK(made == 5 * ngpus);   // points, skip, accel, phi, scratch per device
    set_env("1", nullptr);
    made = sweep("nbody_field", [&] { c.open(ngpus); }, [&] { return nbody_field(c.pts.data(), c.m, nullptr, nullptr, c.phi.data()); },
                 [&] { c.run(false, false, true); });
    CHECK(made == 2 * ngpus);   // points, phi
  }
  set_env(nullptr, nullptr);
  printf("field_sanity ok\n");
  return 0;
}
