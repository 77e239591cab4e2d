// snap_sanity.cpp — TEST INFRASTRUCTURE (tests/test_snap_host_sanitizers.py): drives nbody_snap(_d), nbody_snap_rows(_d) and
// nbody_step_hermite6(_d) of the library's host code (point_sums.cpp, hermite.cpp and hermite6.cpp beside context.cpp, comm.cpp,
// mailbox.cpp, energy.cpp) against tests/host_stub/hip_stub.cpp, snap_stub.cpp, hermite_stub.cpp and hermite6_stub.cpp under
// AddressSanitizer + UBSan.  What it checks is the host's logic: the division of the points over the devices and the rows of a window
// over them, the upload of points, point velocities, point accelerations and skip indices, the copy-back offsets of each of the three
// outputs, the opening jerk rows pass on every device's own rows, the gather of all N accelerations (and velocities) to every device,
// the rows form's offset into the three source arrays, the choice of the source split, the scratch size for nine sums and the
// batches, the argument checks, lifetimes at shutdown and the failure paths; and of the integrator the buffers of a call, the order
// of its gathers and the same state on one and three devices.  snap_stub.cpp states the values expected here.
// It covers rows and points, m = 1, 255, 256, 257, 5000, skip present and absent, each output NULL in turn, one and three stub devices
// with ragged slices, row windows across both device boundaries, the source split forced and automatic, the batched path under a small
// scratch bound, every NBODY_ERR_ARG case, three Hermite-6 steps and the failure sweep of sanity_common.hpp.
#include <string.h>

#define SANITY_NAME "snap_sanity"
#include "sanity_common.hpp"

static const SplitEnv env = {"NBODY_SNAP_SPLIT", "NBODY_SNAP_SCRATCH_MB"};
static const SplitEnv jerk_env = {"NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"};

static int snap_at(const float* p, const float* u, const float* g, int m, const int* sk, float* a, float* j, float* s) { return nbody_snap(p, u, g, m, sk, a, j, s); }
static int snap_at(const double* p, const double* u, const double* g, int m, const int* sk, double* a, double* j, double* s) { return nbody_snap_d(p, u, g, m, sk, a, j, s); }
static int snap_rows(int f, int m, float* a, float* j, float* s) { return nbody_snap_rows(f, m, a, j, s); }
static int snap_rows(int f, int m, double* a, double* j, double* s) { return nbody_snap_rows_d(f, m, a, j, s); }
static int hermite6(float, double dt, int k) { return nbody_step_hermite6((float)dt, k); }
static int hermite6(double, double dt, int k) { return nbody_step_hermite6_d(dt, k); }
template <typename T> int download(std::vector<T>& pos, std::vector<T>& vel);
template <> int download<float>(std::vector<float>& pos, std::vector<float>& vel) { BodySystem b = {pos.data(), vel.data()}; return nbody_download(&b); }
template <> int download<double>(std::vector<double>& pos, std::vector<double>& vel) { BodySystemD b = {pos.data(), vel.data()}; return nbody_download_d(&b); }

// the shared fixture's bodies, points and skip indices, with velocities and accelerations for the points: small integers everywhere, so
// that every value of snap_stub.cpp is exact in either precision
template <typename T>
struct Case : Fixture<T> {
  using Fixture<T>::n; using Fixture<T>::m; using Fixture<T>::pos; using Fixture<T>::vel; using Fixture<T>::pts; using Fixture<T>::skip;
  std::vector<T> pvel, pacc, out[3];
  int nb, out_rows;
  Case(int n_, int m_) : Fixture<T>(n_, m_), pvel((size_t)m_ * 4), pacc((size_t)m_ * 4), nb(stub::blocks_of(n_)), out_rows(std::max(n_, m_)) {
    for (auto& o : out) o.resize((size_t)out_rows * 4);
    for (int j = 0; j < n; ++j) this->set(vel, j, (T)((j * 7) % 11), (T)(j % 5), (T)2, (T)(j % 31));
    for (int p = 0; p < m; ++p) {
      this->set(pvel, p, (T)(p % 3), (T)(p % 4), (T)1, (T)(p % 1000));
      this->set(pacc, p, (T)(p % 5), (T)(p % 7), (T)1, (T)(p % 13));
    }
  }
  // the stub's six jerk values for the query (me, mv, sk): its accel is the acceleration word a snap call gives a row
  void jerk_of(const T* me, const T* mv, int sk, T q6[6]) const {
    double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nb; ++b) {
      const size_t j0 = 4 * (size_t)b * stub::kBlock, jn = 4 * (size_t)(n - 1);
      const bool last = b == nb - 1;
      q[0] += (double)(T)(pos[j0] - me[0]);
      q[1] += (double)(T)(vel[j0] - mv[0]);
      q[2] += (double)(T)((T)sk + (last ? pos[jn] : (T)0));
      q[3] += (double)(T)(mv[1] + (last ? vel[jn] : (T)0));
      q[4] += (double)me[3];
      q[5] += (double)mv[3];
    }
    for (int c = 0; c < 6; ++c) q6[c] = (T)q[c];
  }
  void acc_of_row(int i, T a[4]) const {
    T q6[6];
    jerk_of(&pos[4 * (size_t)i], &vel[4 * (size_t)i], i, q6);
    a[0] = q6[0]; a[1] = q6[1]; a[2] = q6[2]; a[3] = (T)0;
  }
  // the stub's nine values for the query (me, mv, ma, sk)
  void expect(const T* me, const T* mv, const T* ma, int sk, T q9[9]) const {
    jerk_of(me, mv, sk, q9);
    T an[4];
    acc_of_row(n - 1, an);
    double q[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < nb; ++b) {
      T ab[4];
      acc_of_row(b * stub::kBlock, ab);
      q[0] += (double)(T)(ab[0] - ma[0]);
      q[1] += (double)(T)(ma[1] + (b == nb - 1 ? an[0] : (T)0));
      q[2] += (double)ma[3];
    }
    for (int c = 0; c < 3; ++c) q9[6 + c] = (T)q[c];
  }
  void check(int k, const T* me, const T* mv, const T* ma, int sk, const bool (&want)[3]) const {
    T q9[9];
    expect(me, mv, ma, sk, q9);
    for (int o = 0; o < 3; ++o) {
      const T* g = &out[o][4 * (size_t)k];
      if (want[o]) CHECK(g[0] == q9[3 * o] && g[1] == q9[3 * o + 1] && g[2] == q9[3 * o + 2] && g[3] == (T)0);
      else CHECK(g[0] == (T)kMark && g[3] == (T)kMark);
    }
  }
  void mark_all() { for (auto& o : out) mark(o); }
  void nothing_after(int cnt) const { for (const auto& o : out) CHECK(nothing_beyond(o, 4 * (size_t)cnt)); }
  // points [p0, p0 + cnt) of the case, with or without skip and the outputs asked for
  void run(bool with_skip, bool wa = true, bool wj = true, bool ws = true, int p0 = 0, int cnt = -1) {
    if (cnt < 0) cnt = m - p0;
    const bool want[3] = {wa, wj, ws};
    mark_all();
    OK(snap_at(pts.data() + 4 * (size_t)p0, pvel.data() + 4 * (size_t)p0, pacc.data() + 4 * (size_t)p0, cnt, with_skip ? skip.data() + p0 : nullptr,
               wa ? out[0].data() : nullptr, wj ? out[1].data() : nullptr, ws ? out[2].data() : nullptr));
    for (int k = 0; k < cnt; ++k) {
      const int p = p0 + k;
      check(k, &pts[4 * (size_t)p], &pvel[4 * (size_t)p], &pacc[4 * (size_t)p], with_skip ? skip[(size_t)p] : -1, want);
    }
    nothing_after(cnt);
  }
  // rows [first, first + cnt) of the state in pos / vel
  void run_rows(int first = 0, int cnt = -1, bool wa = true, bool wj = true, bool ws = true) {
    if (cnt < 0) cnt = n - first;
    const bool want[3] = {wa, wj, ws};
    mark_all();
    OK(snap_rows(first, cnt, wa ? out[0].data() : nullptr, wj ? out[1].data() : nullptr, ws ? out[2].data() : nullptr));
    for (int k = 0; k < cnt; ++k) {
      T ai[4];
      acc_of_row(first + k, ai);
      check(k, &pos[4 * (size_t)(first + k)], &vel[4 * (size_t)(first + k)], ai, first + k, want);
    }
    nothing_after(cnt);
  }
  void run_all() {
    run(false);
    run(true);
    run(true, false, true, true);    // each output NULL in turn
    run(false, true, false, true);
    run(true, true, true, false);
    run(false, false, false, true);  // the snap alone
    if (m > 2) run(true, true, true, true, 1, m - 2);
    run_rows();
    if (n > 2) {
      run_rows(1, n - 2);
      run_rows(n - 1, 1, false, true, true);
      run_rows(n / 4, n / 2 + 1, true, false, true);   // across both boundaries of three devices
      run_rows(0, n, true, true, false);
    }
  }
};

template <typename T>
static void shapes(int n, int ngpus) {
  for (int m : kShapeM) {
    Case<T> c(n, m);
    c.open(ngpus);
    for_splits(env, {nullptr, "0", "1", "2", "3", "1000"}, [&] { c.run_all(); });
    if (m == 257) for_splits(jerk_env, {"2"}, [&] { c.run_all(); });   // the opening pass split too
    SHUTDOWN();
  }
}

// three Hermite-6 steps: the state after them, fourth values carried; one call and three
template <typename T>
static void hermite_state(int n, int ngpus, int calls, std::vector<T>& pos, std::vector<T>& vel) {
  Case<T> c(n, 1);
  c.open(ngpus);
  for (int k = 0; k < calls; ++k) OK(hermite6(T(), 0.0078125, 3 / calls));
  pos.resize(c.pos.size()); vel.resize(c.vel.size());
  OK(download<T>(pos, vel));
  for (int j = 0; j < n; ++j) CHECK(pos[4 * (size_t)j + 3] == c.pos[4 * (size_t)j + 3] && vel[4 * (size_t)j + 3] == c.vel[4 * (size_t)j + 3]);
  CHECK(pos != c.pos && vel != c.vel);
  long long done = 0;
  OK(nbody_get_info(NBODY_INFO_STEPS_DONE, &done));
  CHECK(done == 3);
  SHUTDOWN();
}

template <typename T>
static void hermite_steps(int n) {
  std::vector<T> p1, v1, p3, v3, q1, w1;
  hermite_state<T>(n, 1, 1, p1, v1);
  hermite_state<T>(n, 1, 3, q1, w1);   // three restarted calls: defined, and run
  if (three_devices() && n >= 3) {
    hermite_state<T>(n, 3, 1, p3, v3);
    CHECK(p1 == p3 && v1 == v3);       // the gathers brought every device what one device has
    env.set("2", nullptr);
    hermite_state<T>(n, 3, 1, p3, v3);
    env.set(nullptr, nullptr);
    CHECK(p1 == p3 && v1 == v3);
  }
}

int main() {
  {
    float one[4] = {0, 0, 0, 0}, a[4] = {5, 5, 5, 5};
    double oned[4] = {0, 0, 0, 0}, ad[4] = {5, 5, 5, 5};
    CHECK(nbody_snap(one, one, one, 1, nullptr, a, a, a) == NBODY_ERR_NOT_INIT && nbody_snap_d(oned, oned, oned, 1, nullptr, ad, ad, ad) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_snap_rows(0, 1, a, a, a) == NBODY_ERR_NOT_INIT && nbody_snap_rows_d(0, 1, ad, ad, ad) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_step_hermite6(0.01f, 1) == NBODY_ERR_NOT_INIT && nbody_step_hermite6_d(0.01, 1) == NBODY_ERR_NOT_INIT);
    CHECK(a[0] == 5 && a[3] == 5 && ad[0] == 5 && ad[3] == 5);
  }

  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 x 3, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 1000, 2085}, shapes<float>, shapes<double>);

  // ---- the batched path: 69 blocks of per-block sums per query against 1 MB, fp32: 69 x 36 B = 2484 B, batches of 256 queries; a
  // ---- window of rows across the devices' boundary 23333 | 23334 ----
  for_device_counts([](int ngpus) {
    Case<float> c(70000, 2000);
    c.open(ngpus);
    for (const char* split : {(const char*)nullptr, "7", "69"}) {
      env.set(split, "1");
      c.run(true);
      c.run(false, false, true, true, 100, 1500);
      c.run_rows(22500, 1500);
    }
    env.set(nullptr, "0");    // not one workgroup's queries fit: no split
    c.run(true);
    env.set("5", "0");
    c.run_rows(23000, 700, false, true, true);
    SHUTDOWN();
  });
  {
    Case<double> c(70000, 600);   // 69 x 72 B = 4968 B per query: batches of 0 — 211 queries fit, not one workgroup: no split
    c.open(1);
    env.set(nullptr, "1");
    c.run(true);
    env.set(nullptr, "2");        // 422 fit: batches of 256
    c.run(true);
    c.run_rows(100, 600);
    SHUTDOWN();
  }
  env.set(nullptr, nullptr);

  // ---- three Hermite-6 steps, both precisions, one device and three ----
  hermite_steps<float>(2085);
  hermite_steps<double>(1000);

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(2085, 300);
    c.open(three_devices() ? 3 : 1);
    float *pts = c.pts.data(), *pv = c.pvel.data(), *pa = c.pacc.data(), *a = c.out[0].data(), *j = c.out[1].data(), *s = c.out[2].data();
    c.mark_all();
    CHECK(nbody_snap(nullptr, pv, pa, 300, nullptr, a, j, s) == NBODY_ERR_ARG);
    CHECK(nbody_snap(pts, nullptr, pa, 300, nullptr, a, j, s) == NBODY_ERR_ARG);
    CHECK(nbody_snap(pts, pv, nullptr, 300, nullptr, a, j, s) == NBODY_ERR_ARG);
    CHECK(nbody_snap(pts, pv, pa, 0, nullptr, a, j, s) == NBODY_ERR_ARG);
    CHECK(nbody_snap(pts, pv, pa, -1, nullptr, a, j, s) == NBODY_ERR_ARG);
    CHECK(nbody_snap(pts, pv, pa, 300, nullptr, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    for (int bad : refused_skips(2085)) CHECK(nbody_snap(pts, pv, pa, 300, c.skip_with(299, bad).data(), a, j, s) == NBODY_ERR_ARG);
    CHECK(nbody_snap_rows(0, 300, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    for (const Window& w : refused_windows(2085, 300)) CHECK(nbody_snap_rows(w.first, w.count, a, j, s) == NBODY_ERR_ARG);
    CHECK(nbody_snap_rows(2082, 4, a, j, s) == NBODY_ERR_ARG && nbody_snap_rows(0, 2086, a, j, s) == NBODY_ERR_ARG);
    CHECK(nbody_step_hermite6(0.01f, 0) == NBODY_ERR_ARG && nbody_step_hermite6(0.01f, -2) == NBODY_ERR_ARG);
    CHECK(nbody_step_hermite6(1.0f / 0.0f, 1) == NBODY_ERR_ARG);
    double t = 5.0;
    int steps = 5;
    CHECK(nbody_step_hermite6_adaptive(0.0f, 1.0f, 1e-6f, 1.0f, 10, &t, &steps) == NBODY_ERR_ARG);
    CHECK(nbody_step_hermite6_adaptive(0.04f, 1.0f, 1.0f, 0.5f, 10, &t, &steps) == NBODY_ERR_ARG);
    CHECK(nbody_step_hermite6_adaptive(0.04f, 1.0f, 1e-6f, 1.0f, 0, &t, &steps) == NBODY_ERR_ARG && t == 5.0 && steps == 5);
    c.nothing_after(0);
    std::vector<double> pd(1200, 0.0), ad(1200, 5.0);
    CHECK(nbody_snap_d(pd.data(), pd.data(), pd.data(), 300, nullptr, ad.data(), ad.data(), ad.data()) == NBODY_ERR_STATE && ad[0] == 5.0 && ad[1199] == 5.0);
    CHECK(nbody_snap_rows_d(0, 300, ad.data(), ad.data(), ad.data()) == NBODY_ERR_STATE && nbody_step_hermite6_d(0.01, 1) == NBODY_ERR_STATE && ad[0] == 5.0);
    c.run_all();
    OK(nbody_step_hermite6_adaptive(0.04f, 0.03125f, 0.0078125f, 0.015625f, 2, &t, &steps));
    CHECK(steps == 2 && t > 0.0 && t <= 0.03125);
    SHUTDOWN();
    Case<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_snap(pts, pv, pa, 10, nullptr, a, j, s) == NBODY_ERR_STATE && nbody_snap_rows(0, 10, a, j, s) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a snap call and of a Hermite-6 call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(2085, 700);
    env.set("3", nullptr);
    int split = sweep("nbody_snap split", [&] { c.open(ngpus); },
                      [&] { return nbody_snap(c.pts.data(), c.pvel.data(), c.pacc.data(), c.m, c.skip.data(), c.out[0].data(), c.out[1].data(), c.out[2].data()); },
                      [&] { c.run(true); });
    int rows_split = sweep("nbody_snap_rows split", [&] { c.open(ngpus); }, [&] { return nbody_snap_rows(0, c.n, c.out[0].data(), c.out[1].data(), c.out[2].data()); },
                           [&] { c.run_rows(); });
    env.set("1", nullptr);
    int plain = sweep("nbody_snap", [&] { c.open(ngpus); },
                      [&] { return nbody_snap(c.pts.data(), c.pvel.data(), c.pacc.data(), c.m, nullptr, nullptr, nullptr, c.out[2].data()); },
                      [&] { c.run(false, false, false, true); });
    int rows = sweep("nbody_snap_rows", [&] { c.open(ngpus); }, [&] { return nbody_snap_rows(600, 900, c.out[0].data(), nullptr, nullptr); },
                     [&] { c.run_rows(600, 900, true, false, false); });
    // the unsplit calls allocate no scratch: one buffer fewer per device that takes part; a points call uploads what a rows call reads in place
    CHECK(split > plain && rows_split > rows && split > rows_split && plain > 0 && rows > 0);
    int made = sweep("nbody_step_hermite6", [&] { c.open(ngpus); }, [&] { return nbody_step_hermite6(0.0078125f, 2); }, [&] {});
    CHECK(made > rows);   // the buffers of a call on top of a snap rows call's
  });
  env.set(nullptr, nullptr);
  printf("snap_sanity ok\n");
  return 0;
}
