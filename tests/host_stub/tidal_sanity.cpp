// tidal_sanity.cpp — TEST INFRASTRUCTURE (tests/test_tidal_host_sanitizers.py): drives nbody_tidal(_d) of the library's host code
// (tidal.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp and field.cpp) against tests/host_stub/hip_stub.cpp, tidal_stub.cpp
// and field_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's logic: the division of the points over the devices,
// the upload and copy-back offsets of the six values per point, the choice of the source split, the scratch size and the batches, the
// argument checks, nbody_field calls between tidal calls (the two passes share their query buffers), lifetimes at shutdown and the
// failure paths.  tidal_stub.cpp and field_stub.cpp state the values expected here.
#include <string.h>

#define SANITY_NAME "tidal_sanity"
#include "sanity_common.hpp"

static void set_env(const char* split, const char* scratch_mb) {
  if (split) setenv("NBODY_TIDAL_SPLIT", split, 1); else unsetenv("NBODY_TIDAL_SPLIT");
  if (scratch_mb) setenv("NBODY_TIDAL_SCRATCH_MB", scratch_mb, 1); else unsetenv("NBODY_TIDAL_SCRATCH_MB");
}

static int tidal(const float* p, int m, const int* sk, float* t) { return nbody_tidal(p, m, sk, t); }
static int tidal(const double* p, int m, const int* sk, double* t) { return nbody_tidal_d(p, m, sk, t); }
static int field(const float* p, int m, const int* sk, float* a, float* phi) { return nbody_field(p, m, sk, a, phi); }
static int field(const double* p, int m, const int* sk, double* a, double* phi) { return nbody_field_d(p, m, sk, a, phi); }

// small integers everywhere: every sum of tidal_stub.cpp is exact in either precision
template <typename T>
struct Case {
  int n, m;
  std::vector<T> pos, vel, pts, out, phi;
  std::vector<int> skip;
  Case(int n_, int m_) : n(n_), m(m_), pos((size_t)n_ * 4), vel((size_t)n_ * 4, (T)0), pts((size_t)m_ * 4), out((size_t)m_ * 6), phi((size_t)m_), skip((size_t)m_) {
    for (int j = 0; j < n; ++j) { pos[4 * (size_t)j] = (T)(j % 13); pos[4 * (size_t)j + 1] = (T)(j % 7); pos[4 * (size_t)j + 2] = (T)1; pos[4 * (size_t)j + 3] = (T)1; }
    for (int p = 0; p < m; ++p) {
      pts[4 * (size_t)p] = (T)(p % 17); pts[4 * (size_t)p + 1] = (T)(p % 5); pts[4 * (size_t)p + 2] = (T)3; pts[4 * (size_t)p + 3] = (T)p;
      skip[(size_t)p] = p % 3 == 0 ? -1 : (int)(((long long)p * 7919) % n);
    }
  }
  void open(int ngpus) { OK(nbody_init(n, ngpus, sizeof(T) == 8, 0)); OK(upload<T>(pos, vel)); }
  // points [p0, p0 + cnt) of the case, with or without skip
  void run(bool with_skip, int p0 = 0, int cnt = -1) {
    if (cnt < 0) cnt = m - p0;
    const T mark = (T)-77;
    std::fill(out.begin(), out.end(), mark);
    OK(tidal(pts.data() + 4 * (size_t)p0, cnt, with_skip ? skip.data() + p0 : nullptr, out.data()));
    const int nb = (n + 1023) / 1024;
    const double s3 = 3.0 * (double)nb;
    for (int k = 0; k < cnt; ++k) {
      const int p = p0 + k;
      double q0 = 0.0, q1 = 0.0;
      for (int b = 0; b < nb; ++b) { q0 += (double)(T)((T)((b * 1024) % 13) - (T)(p % 17)); q1 += (double)(T)((T)(p % 5) + (T)b); }
      const double q2 = (double)nb * (double)(with_skip ? skip[(size_t)p] : -1) + (double)((n - 1) % 13);
      const T* t = out.data() + 6 * (size_t)k;
      CHECK(t[0] == (T)(q0 - s3) && t[1] == (T)(q1 - s3) && t[2] == (T)(q2 - s3));
      CHECK(t[3] == (T)((double)nb * (double)p) && t[4] == (T)((double)nb * (double)(nb - 1) / 2.0) && t[5] == (T)nb);
    }
    for (size_t k = 6 * (size_t)cnt; k < out.size(); ++k) CHECK(out[k] == mark);   // nothing beyond the points asked for
  }
  // a field call on the same context: phi alone, of field_stub.cpp
  void run_field() {
    OK(field(pts.data(), m, skip.data(), nullptr, phi.data()));
    const int nb = (n + 1023) / 1024;
    for (int p = 0; p < m; ++p) CHECK(phi[(size_t)p] == (T)(0.0 - (double)nb * (double)p));
  }
  void run_all() {
    run(false);
    run_field();
    run(true);
    if (m > 2) run(true, 1, m - 2);
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
  float one[4] = {0, 0, 0, 0}, out[6] = {5, 5, 5, 5, 5, 5};
  double oned[4] = {0, 0, 0, 0}, outd[6] = {5, 5, 5, 5, 5, 5};
  CHECK(nbody_tidal(one, 1, nullptr, out) == NBODY_ERR_NOT_INIT && nbody_tidal_d(oned, 1, nullptr, outd) == NBODY_ERR_NOT_INIT);
  CHECK(out[0] == 5 && outd[5] == 5);

  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 + 695 + 695, 1000 = 333 + 333 + 334) ----
  for (int n : {1, 1000, 2085}) {
    shapes<float>(n, 1);
    if (three_devices && n >= 3) shapes<float>(n, 3);
  }
  shapes<double>(2085, 1);
  if (three_devices) shapes<double>(1000, 3);

  // ---- the batched path: 69 blocks x 28 B = 1932 B of per-block sums per point against 1 MB: batches of 512 points (fp32) ----
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
    Case<double> c(70000, 1000);   // 3864 B per point: batches of 256
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
    std::fill(c.out.begin(), c.out.end(), -77.f);
    CHECK(nbody_tidal(nullptr, 300, nullptr, c.out.data()) == NBODY_ERR_ARG);
    CHECK(nbody_tidal(pts, 300, nullptr, nullptr) == NBODY_ERR_ARG);
    CHECK(nbody_tidal(pts, 0, nullptr, c.out.data()) == NBODY_ERR_ARG);
    CHECK(nbody_tidal(pts, -1, nullptr, c.out.data()) == NBODY_ERR_ARG);
    for (int bad : {2085, -2, 1 << 30}) {
      std::vector<int> sk = c.skip;
      sk[299] = bad;
      CHECK(nbody_tidal(pts, 300, sk.data(), c.out.data()) == NBODY_ERR_ARG);
    }
    for (float v : c.out) CHECK(v == -77.f);
    std::vector<int> edge = c.skip;
    edge[0] = 2084; edge[299] = 0;
    OK(nbody_tidal(pts, 300, edge.data(), c.out.data()));
    std::vector<double> pd(1200, 0.0), td(1800, 5.0);
    CHECK(nbody_tidal_d(pd.data(), 300, nullptr, td.data()) == NBODY_ERR_STATE && td[0] == 5.0 && td[1799] == 5.0);
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_tidal(pts, 10, nullptr, c.out.data()) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a tidal call, one device and three, split (scratch) and not ----
  for (int ngpus : {1, 3}) {
    if (ngpus > 1 && !three_devices) continue;
    Case<float> c(2085, 700);
    set_env("3", nullptr);
    int made = sweep("nbody_tidal split", [&] { c.open(ngpus); }, [&] { return nbody_tidal(c.pts.data(), c.m, c.skip.data(), c.out.data()); },
                     [&] { c.run(true); });
    CHECK(made == 4 * ngpus);   // points, skip, tensor, scratch per device
    set_env("1", nullptr);
    made = sweep("nbody_tidal", [&] { c.open(ngpus); }, [&] { return nbody_tidal(c.pts.data(), c.m, nullptr, c.out.data()); },
                 [&] { c.run(false); });
    CHECK(made == 2 * ngpus);   // points, tensor
  }
  set_env(nullptr, nullptr);
  printf("tidal_sanity ok\n");
  return 0;
}
