// hermite_sanity.cpp — TEST INFRASTRUCTURE (tests/test_hermite_host_sanitizers.py): drives nbody_step_hermite(_d), nbody_min_aarseth and
// nbody_step_hermite_adaptive(_d) of the library's host code (hermite.cpp and point_sums.cpp beside context.cpp, comm.cpp, mailbox.cpp,
// energy.cpp) against tests/host_stub/hip_stub.cpp, jerk_stub.cpp and hermite_stub.cpp under AddressSanitizer + UBSan.  What it checks is
// the host's logic: the buffers of a call on every device, the own slice's offset into the live position buffer, the predicted state
// reaching every device (positions and velocities gathered anew in every step), the two sets of (a, j) words changing roles, the
// jerk pass's split and batches without a copy back, the ranks' best words, the adaptive loop, the argument checks, lifetimes at shutdown
// and the failure paths.  The expectations come from a model of the two stubs, operation for operation: jerk_stub.cpp's values of a row
// (they depend on the state of ALL bodies: a device that evaluated on a stale slice is found out) under hermite_stub.cpp's arithmetic.
// It covers N = 1, 1000 and 2085 on one stub device and three with ragged slices, calls of 1 and 3 steps, the source split forced and
// automatic, the batched path under a small scratch bound, the adaptive loop hitting max_steps and hitting t_end, nbody_min_aarseth with
// either pointer NULL, Hermite calls interleaved with nbody_step and nbody_jerk_rows on one context, every NBODY_ERR_ARG case and the
// failure sweep of sanity_common.hpp.
#include <math.h>
#include <string.h>

#include <limits>

#define SANITY_NAME "hermite_sanity"
#include "sanity_common.hpp"

static const SplitEnv env = {"NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"};

static int hermite(float, double dt, int k) { return nbody_step_hermite((float)dt, k); }
static int hermite(double, double dt, int k) { return nbody_step_hermite_d(dt, k); }
static int adaptive(float, double eta, double t_end, double lo, double hi, int ms, double* t, int* s) {
  return nbody_step_hermite_adaptive((float)eta, (float)t_end, (float)lo, (float)hi, ms, t, s);
}
static int adaptive(double, double eta, double t_end, double lo, double hi, int ms, double* t, int* s) {
  return nbody_step_hermite_adaptive_d(eta, t_end, lo, hi, ms, t, s);
}
static int jerk_rows(int f, int m, float* a, float* j) { return nbody_jerk_rows(f, m, a, j); }
static int jerk_rows(int f, int m, double* a, double* j) { return nbody_jerk_rows_d(f, m, a, j); }
static int step(float, double dt) { return nbody_step((float)dt, 1); }
static int step(double, double dt) { return nbody_step_d(dt, 1); }
template <typename T> int download(std::vector<T>& pos, std::vector<T>& vel);
template <> int download<float>(std::vector<float>& pos, std::vector<float>& vel) { BodySystem b = {pos.data(), vel.data()}; return nbody_download(&b); }
template <> int download<double>(std::vector<double>& pos, std::vector<double>& vel) { BodySystemD b = {pos.data(), vel.data()}; return nbody_download_d(&b); }

// the model: the state on the host, jerk_stub.cpp's (a, j) of every row of it, hermite_stub.cpp's step
template <typename T>
struct Model {
  int n, nb, k = 0;
  std::vector<T> pos, vel, x0, v0, a[2], j[2];
  Model(const std::vector<T>& p, const std::vector<T>& v) : n((int)(p.size() / 4)), nb(stub::blocks_of(n)), pos(p), vel(v) {
    for (int i = 0; i < 2; ++i) { a[i].resize(p.size()); j[i].resize(p.size()); }
    eval(0);
  }
  void eval(int to) {
    for (int i = 0; i < n; ++i) {
      const T* me = &pos[4 * (size_t)i];
      const T* mv = &vel[4 * (size_t)i];
      double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int b = 0; b < nb; ++b) {
        const size_t j0 = 4 * (size_t)b * stub::kBlock, jn = 4 * (size_t)(n - 1);
        const bool last = b == nb - 1;
        q[0] += (double)(T)(pos[j0] - me[0]);
        q[1] += (double)(T)(vel[j0] - mv[0]);
        q[2] += (double)(T)((T)i + (last ? pos[jn] : (T)0));
        q[3] += (double)(T)(mv[1] + (last ? vel[jn] : (T)0));
        q[4] += (double)me[3];
        q[5] += (double)mv[3];
      }
      for (int c = 0; c < 3; ++c) { a[to][4 * (size_t)i + c] = (T)q[c]; j[to][4 * (size_t)i + c] = (T)q[3 + c]; }
      a[to][4 * (size_t)i + 3] = (T)0; j[to][4 * (size_t)i + 3] = (T)0;
    }
  }
  void step(T h) {
    const T h2 = h * h, c2 = h2 * (T)0.5, h3 = h2 * h, c3 = h3 / (T)6, hh = h * (T)0.5, c12 = h2 / (T)12;
    x0 = pos; v0 = vel;
    const std::vector<T>&a0 = a[k], &j0 = j[k];
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < 3; ++c) {
        const size_t e = 4 * (size_t)i + c;
        pos[e] = std::fma(c3, j0[e], std::fma(c2, a0[e], std::fma(h, v0[e], x0[e])));
        vel[e] = std::fma(c2, j0[e], std::fma(h, a0[e], v0[e]));
      }
    eval(k ^ 1);
    const std::vector<T>&a1 = a[k ^ 1], &j1 = j[k ^ 1];
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < 3; ++c) {
        const size_t e = 4 * (size_t)i + c;
        const T dj = j0[e] - j1[e], sa = a0[e] + a1[e], da = a0[e] - a1[e];
        const T v1 = std::fma(c12, dj, std::fma(hh, sa, v0[e]));
        const T sv = v0[e] + v1;
        vel[e] = v1;
        pos[e] = std::fma(c12, da, std::fma(hh, sv, x0[e]));
      }
    k ^= 1;
  }
  void best(double* q, int* row) const {
    *q = std::numeric_limits<double>::infinity(); *row = -1;
    for (int i = 0; i < n; ++i) {
      const T* ai = &a[k][4 * (size_t)i];
      const T* ji = &j[k][4 * (size_t)i];
      const double ax = (double)ai[0], ay = (double)ai[1], az = (double)ai[2], jx = (double)ji[0], jy = (double)ji[1], jz = (double)ji[2];
      const double a2 = (ax * ax + ay * ay) + az * az, j2 = (jx * jx + jy * jy) + jz * jz;
      const double qi = a2 / j2;
      if (qi < *q) { *q = qi; *row = i; }
    }
  }
  void run_adaptive(double eta, double t_end, double lo, double hi, int max_steps, double* t_out, int* steps_out) {
    double t = 0.0;
    int steps = 0;
    while (t < t_end && steps < max_steps) {
      double q;
      int row;
      best(&q, &row);
      double h = eta * sqrt(q);
      h = h > hi ? hi : h;
      h = h < lo ? lo : h;
      if (t + h > t_end) h = t_end - t;
      const T dt = (T)h;
      step(dt);
      t += (double)dt;
      ++steps;
    }
    *t_out = t; *steps_out = steps;
  }
};

// the shared fixture's bodies with velocities: small integers, the w words tag the rows (jerk_stub.cpp reads them)
template <typename T>
struct Case : Fixture<T> {
  using Fixture<T>::n; using Fixture<T>::pos; using Fixture<T>::vel;
  std::vector<T> gp, gv, acc, jerk;
  explicit Case(int n_) : Fixture<T>(n_, 1), gp((size_t)n_ * 4), gv((size_t)n_ * 4), acc((size_t)n_ * 4), jerk((size_t)n_ * 4) {
    for (int j = 0; j < n; ++j) this->set(vel, j, (T)((j * 7) % 11), (T)(j % 5), (T)2, (T)(j % 31));
  }
  void reset() { OK(upload<T>(pos, vel)); }
  void fetch() { OK(download<T>(gp, gv)); }
  // the state on the device is the model's, bit for bit (memcmp: a NaN would be a finding, not a pass)
  void same_state(const Model<T>& m) {
    fetch();
    CHECK(!memcmp(gp.data(), m.pos.data(), gp.size() * sizeof(T)) && !memcmp(gv.data(), m.vel.data(), gv.size() * sizeof(T)));
  }
  // a fresh upload, `calls` calls of `steps` steps each: every call is a restart of the model too
  void run(int calls, int steps, double dt) {
    reset();
    Model<T> m(pos, vel);
    for (int c = 0; c < calls; ++c) {
      OK(hermite(T(), dt, steps));
      if (c) m = Model<T>(m.pos, m.vel);
      for (int s = 0; s < steps; ++s) m.step((T)dt);
    }
    same_state(m);
    for (int i = 0; i < n; ++i) CHECK(gp[4 * (size_t)i + 3] == pos[4 * (size_t)i + 3] && gv[4 * (size_t)i + 3] == vel[4 * (size_t)i + 3]);
  }
  void run_min() {
    Model<T> m(gp_now(), gv);
    double q = -1.0, wq;
    int row = -2, wrow;
    m.best(&wq, &wrow);
    OK(nbody_min_aarseth(&q, &row));
    CHECK(q == wq && row == wrow);
    q = -1.0; row = -2;
    OK(nbody_min_aarseth(&q, nullptr));
    OK(nbody_min_aarseth(nullptr, &row));
    CHECK(q == wq && row == wrow);
    same_state(m);   // the call has changed nothing
  }
  const std::vector<T>& gp_now() { fetch(); return gp; }
  void run_adaptive(double eta, double t_end, double lo, double hi, int max_steps, bool ends) {
    eta = (double)(T)eta; t_end = (double)(T)t_end; lo = (double)(T)lo; hi = (double)(T)hi;   // as the entry point of T receives them
    reset();
    Model<T> m(pos, vel);
    double t = -1.0, wt;
    int steps = -1, wsteps;
    m.run_adaptive(eta, t_end, lo, hi, max_steps, &wt, &wsteps);
    OK(adaptive(T(), eta, t_end, lo, hi, max_steps, &t, &steps));
    CHECK(t == wt && steps == wsteps && (ends ? t >= t_end : (t < t_end && steps == max_steps)));
    same_state(m);
    reset();
    OK(adaptive(T(), eta, t_end, lo, hi, max_steps, nullptr, nullptr));
    same_state(m);
  }
  // Hermite calls between nbody_step and nbody_jerk_rows calls on one context: every one sees the state the last one left
  void run_interleaved() {
    reset();
    OK(hermite(T(), 0.0078125, 1));
    OK(step(T(), 0.0078125));
    OK(nbody_sync());
    Model<T> m(gp_now(), gv);
    OK(jerk_rows(0, n, acc.data(), jerk.data()));
    CHECK(!memcmp(acc.data(), m.a[0].data(), acc.size() * sizeof(T)) && !memcmp(jerk.data(), m.j[0].data(), jerk.size() * sizeof(T)));
    OK(hermite(T(), 0.0078125, 3));
    for (int s = 0; s < 3; ++s) m.step((T)0.0078125);
    same_state(m);
    OK(jerk_rows(0, n, acc.data(), jerk.data()));          // the corrected state of ALL bodies, on every device
    Model<T> after(m.pos, m.vel);
    CHECK(!memcmp(acc.data(), after.a[0].data(), acc.size() * sizeof(T)) && !memcmp(jerk.data(), after.j[0].data(), jerk.size() * sizeof(T)));
    OK(step(T(), 0.0078125));
    OK(hermite(T(), -0.0078125, 1));                        // a negative dt
    OK(nbody_sync());
    run_min();
  }
  void run_all() {
    run(1, 1, 0.0078125);
    run(1, 3, 0.0078125);
    run(2, 1, 0.01);
    run_min();
  }
};

template <typename T>
static void shapes(int n, int ngpus) {
  Case<T> c(n);
  c.open(ngpus);
  long long done = -1;
  for_splits(env, {nullptr, "1", "2", "3", "1000"}, [&] { c.run_all(); });
  OK(nbody_get_info(NBODY_INFO_STEPS_DONE, &done));
  CHECK(done == 5 * 6);
  c.run_interleaved();
  env.set("2", nullptr);
  c.run_interleaved();
  env.set(nullptr, nullptr);
  c.run_adaptive(0.5, 0.25, 1e-3, 0.0625, 1000, true);    // to t_end (no step is longer than 1/16: at least four)
  c.run_adaptive(0.5, 0.25, 1e-3, 0.0625, 2, false);      // max_steps
  c.run_adaptive(1e-3, 0.01, 1e-3, 1.0, 1000, true);      // short steps (dt_min or the Aarseth step itself), then the remainder
  SHUTDOWN();
}

int main() {
  {
    double q = 5.0, t = 5.0;
    int row = 5, s = 5;
    CHECK(nbody_step_hermite(0.01f, 1) == NBODY_ERR_NOT_INIT && nbody_step_hermite_d(0.01, 1) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_min_aarseth(&q, &row) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_step_hermite_adaptive(0.1f, 1.f, 0.001f, 1.f, 10, &t, &s) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_step_hermite_adaptive_d(0.1, 1.0, 0.001, 1.0, 10, &t, &s) == NBODY_ERR_NOT_INIT);
    CHECK(q == 5.0 && row == 5 && t == 5.0 && s == 5);
  }

  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 x 3, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 1000, 2085}, shapes<float>, shapes<double>);

  // ---- the batched path: 69 blocks of per-block sums per row against 1 MB, fp32: 69 x 24 B = 1656 B, batches of 512 rows ----
  for_device_counts([](int ngpus) {
    Case<float> c(70000);
    c.open(ngpus);
    for (const char* split : {(const char*)nullptr, "7"}) {
      env.set(split, "1");
      c.run(1, 1, 0.0078125);
    }
    env.set("5", "0");    // not one workgroup's rows fit: no split
    c.run(1, 2, 0.0078125);
    SHUTDOWN();
  });
  env.set(nullptr, nullptr);

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(2085);
    c.open(three_devices() ? 3 : 1);
    double t = 5.0, q = 5.0;
    int s = 5, row = 5;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(nbody_step_hermite(0.01f, 0) == NBODY_ERR_ARG && nbody_step_hermite(0.01f, -1) == NBODY_ERR_ARG);
    CHECK(nbody_step_hermite(inf, 1) == NBODY_ERR_ARG && nbody_step_hermite(-inf, 1) == NBODY_ERR_ARG && nbody_step_hermite(nan, 1) == NBODY_ERR_ARG);
    CHECK(nbody_min_aarseth(nullptr, nullptr) == NBODY_ERR_ARG);
    auto ad = [&](float eta, float t_end, float lo, float hi, int ms) { return nbody_step_hermite_adaptive(eta, t_end, lo, hi, ms, &t, &s); };
    CHECK(ad(0.f, 1.f, 0.001f, 1.f, 10) == NBODY_ERR_ARG && ad(-1.f, 1.f, 0.001f, 1.f, 10) == NBODY_ERR_ARG && ad(nan, 1.f, 0.001f, 1.f, 10) == NBODY_ERR_ARG);
    CHECK(ad(inf, 1.f, 0.001f, 1.f, 10) == NBODY_ERR_ARG);
    CHECK(ad(0.1f, 0.f, 0.001f, 1.f, 10) == NBODY_ERR_ARG && ad(0.1f, -1.f, 0.001f, 1.f, 10) == NBODY_ERR_ARG && ad(0.1f, nan, 0.001f, 1.f, 10) == NBODY_ERR_ARG);
    CHECK(ad(0.1f, inf, 0.001f, 1.f, 10) == NBODY_ERR_ARG);
    CHECK(ad(0.1f, 1.f, 0.f, 1.f, 10) == NBODY_ERR_ARG && ad(0.1f, 1.f, -0.001f, 1.f, 10) == NBODY_ERR_ARG && ad(0.1f, 1.f, nan, 1.f, 10) == NBODY_ERR_ARG);
    CHECK(ad(0.1f, 1.f, 0.001f, 0.0001f, 10) == NBODY_ERR_ARG && ad(0.1f, 1.f, 0.001f, inf, 10) == NBODY_ERR_ARG && ad(0.1f, 1.f, 0.001f, nan, 10) == NBODY_ERR_ARG);
    CHECK(ad(0.1f, 1.f, 0.001f, 1.f, 0) == NBODY_ERR_ARG && ad(0.1f, 1.f, 0.001f, 1.f, -5) == NBODY_ERR_ARG);
    CHECK(nbody_step_hermite_d(0.01, 1) == NBODY_ERR_STATE && nbody_step_hermite_adaptive_d(0.1, 1.0, 0.001, 1.0, 10, &t, &s) == NBODY_ERR_STATE);
    CHECK(t == 5.0 && s == 5 && q == 5.0 && row == 5);
    long long done = -1;
    OK(nbody_get_info(NBODY_INFO_STEPS_DONE, &done));
    CHECK(done == 0);
    c.fetch();
    CHECK(c.gp == c.pos && c.gv == c.vel);   // a refused call has changed nothing in the state
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000);
    d.open(1);
    CHECK(nbody_step_hermite(0.01f, 1) == NBODY_ERR_STATE && nbody_step_hermite_adaptive(0.1f, 1.f, 0.001f, 1.f, 10, &t, &s) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a Hermite call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(2085);
    const int gather = ngpus > 1 ? 1 : 0;   // ts_vel, where the velocities have to travel
    env.set("3", nullptr);
    int made = sweep("nbody_step_hermite split", [&] { c.open(ngpus); }, [&] { return nbody_step_hermite(0.0078125f, 2); }, [&] {
      Model<float> m(c.pos, c.vel);
      m.step(0.0078125f); m.step(0.0078125f);
      c.same_state(m);
    });
    CHECK(made == (8 + gather) * ngpus);   // the ranks' words, (x0, v0), two sets of (a, j), scratch per device
    env.set("1", nullptr);
    made = sweep("nbody_min_aarseth", [&] { c.open(ngpus); }, [&] { double q; return nbody_min_aarseth(&q, nullptr); }, [&] { c.run_min(); });
    CHECK(made == (7 + gather) * ngpus);
    made = sweep("nbody_step_hermite_adaptive", [&] { c.open(ngpus); },
                 [&] { double t; int s; return nbody_step_hermite_adaptive(0.5f, 0.125f, 0.001f, 0.0625f, 10, &t, &s); }, [&] {
                   Model<float> m(c.pos, c.vel);
                   double t;
                   int s;
                   m.run_adaptive(0.5f, 0.125f, 0.001f, 0.0625f, 10, &t, &s);
                   c.same_state(m);
                 });
    CHECK(made == (7 + gather) * ngpus);
  });
  env.set(nullptr, nullptr);
  printf("hermite_sanity ok\n");
  return 0;
}
