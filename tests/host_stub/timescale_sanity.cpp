// timescale_sanity.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py, case `timescale`): drives nbody_timescale_rows(_d),
// nbody_min_timescale(_d) and nbody_step_adaptive(_d) of the library's host code (timescale.cpp beside context.cpp, comm.cpp,
// mailbox.cpp and energy.cpp) against tests/host_stub/hip_stub.cpp and timescale_stub.cpp under AddressSanitizer + UBSan.  What it
// checks is the host's logic: the rows of a window over the devices, the copy-back offsets of the three outputs, the gather of all N
// velocities to every device, the choice of the source split, the scratch size and the batches, the ranks' words of the system form,
// the driver loop, the argument checks, lifetimes at shutdown and the failure paths.  timescale_stub.cpp states the values expected here.
// It covers one and three stub devices with ragged slices, windows of rows across the devices, the source split forced and automatic,
// the batched path under a small scratch bound, the gather of all N velocities on three devices after steps have changed them, every
// NBODY_ERR_ARG case, the driver loop against nbody_step and the failure sweep of sanity_common.hpp.
#include <math.h>
#include <string.h>

#include <limits>

#define SANITY_NAME "timescale_sanity"
#include "sanity_common.hpp"

static const SplitEnv env = {"NBODY_TIMESCALE_SPLIT", "NBODY_TIMESCALE_SCRATCH_MB"};

static int rows(int f, int m, float* t, int* i, float* d) { return nbody_timescale_rows(f, m, t, i, d); }
static int rows(int f, int m, double* t, int* i, double* d) { return nbody_timescale_rows_d(f, m, t, i, d); }
static int system_min(float* t, int* i, int* j, float* d) { return nbody_min_timescale(t, i, j, d); }
static int system_min(double* t, int* i, int* j, double* d) { return nbody_min_timescale_d(t, i, j, d); }
static int adaptive(float, double eta, double t_end, double lo, double hi, int k, double* t, int* s) {
  return nbody_step_adaptive((float)eta, (float)t_end, (float)lo, (float)hi, k, t, s);
}
static int adaptive(double, double eta, double t_end, double lo, double hi, int k, double* t, int* s) {
  return nbody_step_adaptive_d(eta, t_end, lo, hi, k, t, s);
}
static int step(float, double dt) { return nbody_step((float)dt, 1); }
static int step(double, double dt) { return nbody_step_d(dt, 1); }
template <typename T> int download(std::vector<T>& pos, std::vector<T>& vel);
template <> int download<float>(std::vector<float>& pos, std::vector<float>& vel) { BodySystem b = {pos.data(), vel.data()}; return nbody_download(&b); }
template <> int download<double>(std::vector<double>& pos, std::vector<double>& vel) { BodySystemD b = {pos.data(), vel.data()}; return nbody_download_d(&b); }

// small integers everywhere: every value of timescale_stub.cpp is exact in either precision
template <typename T>
struct Case : System<T> {
  using System<T>::n; using System<T>::pos; using System<T>::vel;
  std::vector<T> tau2, d2;
  std::vector<int> idx;
  explicit Case(int n_) : System<T>(n_), tau2((size_t)n_), d2((size_t)n_), idx((size_t)n_) {
    for (int j = 0; j < n; ++j) {
      this->set(pos, j, (T)(j % 13), (T)(j % 7), (T)1, (T)(j % 50));
      vel[4 * (size_t)j] = (T)((j * 7) % 11);
    }
  }
  // what the stub makes of row i of the state in pos / vel
  void expect(int i, T* t, int* ix, T* d) const {
    const T inf = std::numeric_limits<T>::infinity();
    *t = inf; *ix = -1; *d = inf;
    for (int b = 0; b < stub::blocks_of(n); ++b) {
      const int j = stub::candidate(n, pos[4 * (size_t)i + 3], b).j;
      if (j == i) continue;
      const T q = stub::absdiff(pos[4 * (size_t)j], pos[4 * (size_t)i]), v = stub::absdiff(vel[4 * (size_t)j], vel[4 * (size_t)i]);
      if (q < *t) { *t = q; *ix = j; }
      if (v < *d) *d = v;
    }
  }
  // rows [first, first + cnt) with the outputs in `which` (bit 0 tau2, 1 idx, 2 d2min)
  void run(int first = 0, int cnt = -1, int which = 7) {
    if (cnt < 0) cnt = n - first;
    mark(tau2); mark(d2); mark(idx);
    OK(rows(first, cnt, which & 1 ? tau2.data() : nullptr, which & 2 ? idx.data() : nullptr, which & 4 ? d2.data() : nullptr));
    for (int k = 0; k < cnt; ++k) {
      T t, d;
      int ix;
      expect(first + k, &t, &ix, &d);
      CHECK(tau2[(size_t)k] == (which & 1 ? t : (T)kMark));
      CHECK(idx[(size_t)k] == (which & 2 ? ix : kMark));
      CHECK(d2[(size_t)k] == (which & 4 ? d : (T)kMark));
    }
    CHECK(nothing_beyond(tau2, (size_t)cnt) && nothing_beyond(idx, (size_t)cnt) && nothing_beyond(d2, (size_t)cnt));   // nothing beyond the rows asked for
  }
  void run_system() {
    const T inf = std::numeric_limits<T>::infinity();
    T bt = inf, bd = inf;
    int bi = -1, bj = -1;
    for (int i = 0; i < n; ++i) {
      T t, d;
      int ix;
      expect(i, &t, &ix, &d);
      if (t < bt) { bt = t; bi = i; bj = ix; }
      if (d < bd) bd = d;
    }
    T t = (T)kMark, d = (T)kMark;
    int i = kMark, j = kMark;
    OK(system_min(&t, &i, &j, &d));
    CHECK(t == bt && i == bi && j == bj && d == bd);
    i = kMark;
    OK(system_min((T*)nullptr, &i, nullptr, (T*)nullptr));
    CHECK(i == bi);
  }
  void run_all() {
    run();
    run_system();
    if (n > 2) { run(1, n - 2); run(n - 1, 1, 2); run(0, n, 1); run(0, n / 2 + 1, 4); }
  }
  // the state on the device into pos / vel: what the expectations are computed from after steps
  void refresh() { OK(nbody_sync()); OK(download<T>(pos, vel)); }
};

template <typename T>
static void shapes(int n, int ngpus) {
  Case<T> c(n);
  c.open(ngpus);
  for_splits(env, {nullptr, "0", "1", "2", "3", "1000"}, [&] { c.run_all(); });
  // after two steps every device's velocities differ from the upload: all N of them must be gathered anew
  if (n >= 3) {
    OK(step(T(), 0.0078125));
    OK(step(T(), 0.0078125));
    c.refresh();
    env.set("2", nullptr);
    c.run_all();
    env.set(nullptr, nullptr);
    c.run_all();
  }
  SHUTDOWN();
}

template <typename T>
static void driver(int ngpus) {
  const int n = 1000;
  // clamped to one value: three steps of 0.25 and the rest of the way, exactly the steps nbody_step takes
  Case<T> c(n), d(n);
  c.open(ngpus);
  double t = -1.0;
  int k = -1;
  OK(adaptive(T(), 0.5, 0.875, 0.25, 0.25, 100, &t, &k));
  CHECK(k == 4 && t == 0.875);
  c.refresh();
  SHUTDOWN();
  d.open(ngpus);
  for (double dt : {0.25, 0.25, 0.25, 0.125}) OK(step(T(), dt));
  d.refresh();
  CHECK(!memcmp(c.pos.data(), d.pos.data(), c.pos.size() * sizeof(T)) && !memcmp(c.vel.data(), d.vel.data(), c.vel.size() * sizeof(T)));
  SHUTDOWN();
  // the cut-off, and outputs that may be null
  Case<T> e(n);
  e.open(ngpus);
  OK(adaptive(T(), 0.5, 0.875, 0.25, 0.25, 2, &t, &k));
  CHECK(k == 2 && t == 0.5);
  OK(adaptive(T(), 0.5, 0.25, 0.25, 0.25, 2, nullptr, nullptr));
  SHUTDOWN();
  // the formula: one step from the system's minima, rounded once to T
  Case<T> f(n);
  f.open(ngpus);
  T tau2, d2min;
  int i, j;
  OK(system_min(&tau2, &i, &j, &d2min));
  const unsigned eps_bits = 0x3089705Fu;
  float eps;
  memcpy(&eps, &eps_bits, sizeof(eps));
  const double s = (double)d2min + (double)eps, tff2 = s * sqrt(s) / 2.0;
  double h = 0.0078125 * sqrt(std::min((double)tau2, tff2));
  const double dt_min = ldexp(1.0, -20);   // exact in either precision
  h = std::max(dt_min, std::min(h, 1.0));
  OK(adaptive(T(), 0.0078125, 100.0, dt_min, 1.0, 1, &t, &k));
  CHECK(k == 1 && t == (double)(T)h);
  SHUTDOWN();
}

int main() {
  {
    float t[4] = {5, 5, 5, 5};
    double td[4] = {5, 5, 5, 5}, tr = 5.0;
    int ix[4] = {5, 5, 5, 5};
    CHECK(nbody_timescale_rows(0, 4, t, ix, t) == NBODY_ERR_NOT_INIT && nbody_timescale_rows_d(0, 4, td, ix, td) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_min_timescale(t, ix, ix + 1, t + 1) == NBODY_ERR_NOT_INIT && nbody_min_timescale_d(td, ix, ix + 1, td + 1) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_step_adaptive(0.5f, 1.f, 0.1f, 0.2f, 3, &tr, ix) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_step_adaptive_d(0.5, 1., 0.1, 0.2, 3, &tr, ix) == NBODY_ERR_NOT_INIT);
    CHECK(t[0] == 5 && td[1] == 5 && ix[0] == 5 && ix[1] == 5 && tr == 5.0);
  }

  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 x 3, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 2, 1000, 2085}, shapes<float>, shapes<double>);

  // ---- the batched path: 7 chunks x 12 B = 84 B per row against 0.05 MB = 52428 B: batches of 512 rows (fp32); a window across the
  //      devices' boundary 23333 | 23334 ----
  for_device_counts([](int ngpus) {
    Case<float> c(70000);
    c.open(ngpus);
    for (const char* split : {"7", "69"}) {
      env.set(split, "0.05");
      c.run(20000, 5000);
      c.run(23000, 700, 5);
    }
    env.set(nullptr, "0.05");
    c.run(20000, 5000);
    env.set("5", "0");    // not one workgroup's rows fit: no split
    c.run(23000, 700);
    env.set("3", "0.05");
    c.run_system();
    SHUTDOWN();
  });
  {
    Case<double> c(70000);   // 7 chunks x 20 B = 140 B per row: batches of 256
    c.open(1);
    env.set("7", "0.05");
    c.run(100, 1000);
    SHUTDOWN();
  }
  env.set(nullptr, nullptr);

  // ---- the driver loop ----
  for_device_counts([](int ngpus) { driver<float>(ngpus); driver<double>(ngpus); });

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(2085);
    c.open(three_devices() ? 3 : 1);
    std::vector<float> t(2085, (float)kMark);
    std::vector<int> ix(2085, kMark);
    double tr = kMark;
    int st = kMark;
    CHECK(nbody_timescale_rows(0, 2085, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    // this pass's own windows (a rows form only, no count of 300): not sanity_common.hpp's list
    const int bad_rows[][2] = {{-1, 4}, {0, 0}, {0, -2}, {2082, 4}, {2085, 1}, {0, 2086}, {1 << 30, 1 << 30}};
    for (const auto& r : bad_rows) CHECK(nbody_timescale_rows(r[0], r[1], t.data(), ix.data(), t.data()) == NBODY_ERR_ARG);
    CHECK(nbody_min_timescale(nullptr, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float bad[][4] = {{0.f, 1.f, 0.1f, 0.2f}, {-1.f, 1.f, 0.1f, 0.2f}, {0.5f, 0.f, 0.1f, 0.2f}, {0.5f, -1.f, 0.1f, 0.2f}, {0.5f, 1.f, 0.f, 0.2f},
                            {0.5f, 1.f, -0.1f, 0.2f}, {0.5f, 1.f, 0.3f, 0.2f}, {inf, 1.f, 0.1f, 0.2f}, {0.5f, inf, 0.1f, 0.2f}, {0.5f, 1.f, inf, inf},
                            {0.5f, 1.f, 0.1f, inf}, {nan, 1.f, 0.1f, 0.2f}, {0.5f, nan, 0.1f, 0.2f}, {0.5f, 1.f, nan, 0.2f}, {0.5f, 1.f, 0.1f, nan}};
    for (const auto& b : bad) CHECK(nbody_step_adaptive(b[0], b[1], b[2], b[3], 10, &tr, &st) == NBODY_ERR_ARG);
    CHECK(nbody_step_adaptive(0.5f, 1.f, 0.1f, 0.2f, 0, &tr, &st) == NBODY_ERR_ARG && nbody_step_adaptive(0.5f, 1.f, 0.1f, 0.2f, -3, &tr, &st) == NBODY_ERR_ARG);
    CHECK(nothing_beyond(t, 0) && nothing_beyond(ix, 0));
    CHECK(tr == kMark && st == kMark);
    std::vector<double> td(2085, 5.0);
    CHECK(nbody_timescale_rows_d(0, 2085, td.data(), ix.data(), td.data()) == NBODY_ERR_STATE && td[0] == 5.0 && td[2084] == 5.0);
    CHECK(nbody_min_timescale_d(td.data(), ix.data(), ix.data() + 1, td.data() + 1) == NBODY_ERR_STATE && td[0] == 5.0 && ix[0] == kMark);
    CHECK(nbody_step_adaptive_d(0.5, 1., 0.1, 0.2, 3, &tr, &st) == NBODY_ERR_STATE && tr == kMark && st == kMark);
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000);
    d.open(1);
    CHECK(nbody_timescale_rows(0, 1000, t.data(), ix.data(), t.data()) == NBODY_ERR_STATE);
    CHECK(nbody_min_timescale(t.data(), ix.data(), ix.data() + 1, t.data() + 1) == NBODY_ERR_STATE);
    CHECK(nbody_step_adaptive(0.5f, 1.f, 0.1f, 0.2f, 3, &tr, &st) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(2085);
    const int gather = ngpus > 1 ? 1 : 0;   // ts_vel, where the velocities have to travel
    env.set("3", nullptr);
    int made = sweep("nbody_timescale_rows split", [&] { c.open(ngpus); },
                     [&] { return nbody_timescale_rows(0, c.n, c.tau2.data(), c.idx.data(), c.d2.data()); }, [&] { c.run(); });
    CHECK(made == (4 + gather) * ngpus);   // tau2, idx, d2min, scratch per device
    env.set("1", nullptr);
    made = sweep("nbody_timescale_rows", [&] { c.open(ngpus); }, [&] { return nbody_timescale_rows(0, c.n, c.tau2.data(), nullptr, nullptr); },
                 [&] { c.run(0, -1, 1); });
    CHECK(made == (1 + gather) * ngpus);   // tau2
    float t, d;
    int i, j;
    made = sweep("nbody_min_timescale", [&] { c.open(ngpus); }, [&] { return nbody_min_timescale(&t, &i, &j, &d); }, [&] { c.run_system(); });
    CHECK(made == (4 + gather) * ngpus);   // tau2, idx, d2min, the ranks' words
    double tr;
    int st;
    sweep("nbody_step_adaptive", [&] { c.open(ngpus); }, [&] { return nbody_step_adaptive(0.5f, 0.5f, 0.25f, 0.25f, 5, &tr, &st); },
          [&] { CHECK(st == 2 && tr == 0.5); });
  });
  env.set(nullptr, nullptr);
  printf("timescale_sanity ok\n");
  return 0;
}
