// jerk_sanity.cpp — TEST INFRASTRUCTURE (tests/test_jerk_host_sanitizers.py): drives nbody_jerk(_d) and nbody_jerk_rows(_d) of the
// library's host code (point_sums.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp) against tests/host_stub/hip_stub.cpp and
// jerk_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's logic: the division of the points over the devices and
// the rows of a window over them, the upload of points, point velocities and skip indices, the copy-back offsets of each output, the
// gather of all N velocities to every device, the rows form's offset into the sources, the choice of the source split, the scratch size
// and the batches, the argument checks, nbody_field calls between jerk calls (the passes share their buffers), lifetimes at shutdown and
// the failure paths.  jerk_stub.cpp states the values expected here.
// It covers m = 1, 255, 256, 257, 5000, skip present and absent, either output NULL, one and three stub devices with ragged slices, row
// windows across both device boundaries after steps have changed the velocities, the source split forced and automatic, the batched
// path under a small scratch bound, every NBODY_ERR_ARG case and the failure sweep of sanity_common.hpp.
#include <string.h>

#define SANITY_NAME "jerk_sanity"
#include "sanity_common.hpp"

static const SplitEnv env = {"NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"};
static const SplitEnv field_env = {"NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB"};

static int jerk_at(const float* p, const float* u, int m, const int* sk, float* a, float* j) { return nbody_jerk(p, u, m, sk, a, j); }
static int jerk_at(const double* p, const double* u, int m, const int* sk, double* a, double* j) { return nbody_jerk_d(p, u, m, sk, a, j); }
static int jerk_rows(int f, int m, float* a, float* j) { return nbody_jerk_rows(f, m, a, j); }
static int jerk_rows(int f, int m, double* a, double* j) { return nbody_jerk_rows_d(f, m, a, j); }
static int field(const float* p, int m, const int* sk, float* a, float* phi) { return nbody_field(p, m, sk, a, phi); }
static int field(const double* p, int m, const int* sk, double* a, double* phi) { return nbody_field_d(p, m, sk, a, phi); }
static int step(float, double dt) { return nbody_step((float)dt, 1); }
static int step(double, double dt) { return nbody_step_d(dt, 1); }
template <typename T> int download(std::vector<T>& pos, std::vector<T>& vel);
template <> int download<float>(std::vector<float>& pos, std::vector<float>& vel) { BodySystem b = {pos.data(), vel.data()}; return nbody_download(&b); }
template <> int download<double>(std::vector<double>& pos, std::vector<double>& vel) { BodySystemD b = {pos.data(), vel.data()}; return nbody_download_d(&b); }

// the shared fixture's bodies, points and skip indices, with velocities for both: small integers everywhere, so that every value of
// jerk_stub.cpp is exact in either precision (after steps the expectations follow the downloaded state, operation for operation)
template <typename T>
struct Case : Fixture<T> {
  using Fixture<T>::n; using Fixture<T>::m; using Fixture<T>::pos; using Fixture<T>::vel; using Fixture<T>::pts; using Fixture<T>::skip;
  std::vector<T> pvel, acc, jerk, phi;
  int nb, out_rows;
  Case(int n_, int m_) : Fixture<T>(n_, m_), pvel((size_t)m_ * 4), nb(stub::blocks_of(n_)), out_rows(std::max(n_, m_)) {
    acc.resize((size_t)out_rows * 4); jerk.resize((size_t)out_rows * 4); phi.resize((size_t)m_);
    for (int j = 0; j < n; ++j) this->set(vel, j, (T)((j * 7) % 11), (T)(j % 5), (T)2, (T)(j % 31));
    for (int p = 0; p < m; ++p) this->set(pvel, p, (T)(p % 3), (T)(p % 4), (T)1, (T)(p % 1000));
  }
  // the stub's results for the query (me, mv, sk)
  void expect(const T* me, const T* mv, int sk, T a[3], T j[3]) const {
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
    for (int c = 0; c < 3; ++c) { a[c] = (T)q[c]; j[c] = (T)q[3 + c]; }
  }
  void check(int k, const T* me, const T* mv, int sk, bool want_a, bool want_j) const {
    T a[3], j[3];
    expect(me, mv, sk, a, j);
    const T* ga = &acc[4 * (size_t)k];
    const T* gj = &jerk[4 * (size_t)k];
    if (want_a) CHECK(ga[0] == a[0] && ga[1] == a[1] && ga[2] == a[2] && ga[3] == (T)0);
    else CHECK(ga[0] == (T)kMark && ga[3] == (T)kMark);
    if (want_j) CHECK(gj[0] == j[0] && gj[1] == j[1] && gj[2] == j[2] && gj[3] == (T)0);
    else CHECK(gj[0] == (T)kMark && gj[3] == (T)kMark);
  }
  // points [p0, p0 + cnt) of the case, with or without skip and either output
  void run(bool with_skip, bool want_a, bool want_j, int p0 = 0, int cnt = -1) {
    if (cnt < 0) cnt = m - p0;
    mark(acc); mark(jerk);
    OK(jerk_at(pts.data() + 4 * (size_t)p0, pvel.data() + 4 * (size_t)p0, cnt, with_skip ? skip.data() + p0 : nullptr,
               want_a ? acc.data() : nullptr, want_j ? jerk.data() : nullptr));
    for (int k = 0; k < cnt; ++k) {
      const int p = p0 + k;
      check(k, &pts[4 * (size_t)p], &pvel[4 * (size_t)p], with_skip ? skip[(size_t)p] : -1, want_a, want_j);
    }
    CHECK(nothing_beyond(acc, 4 * (size_t)cnt) && nothing_beyond(jerk, 4 * (size_t)cnt));   // nothing beyond the points asked for
  }
  // rows [first, first + cnt) of the state in pos / vel
  void run_rows(int first = 0, int cnt = -1, bool want_a = true, bool want_j = true) {
    if (cnt < 0) cnt = n - first;
    mark(acc); mark(jerk);
    OK(jerk_rows(first, cnt, want_a ? acc.data() : nullptr, want_j ? jerk.data() : nullptr));
    for (int k = 0; k < cnt; ++k) check(k, &pos[4 * (size_t)(first + k)], &vel[4 * (size_t)(first + k)], first + k, want_a, want_j);
    CHECK(nothing_beyond(acc, 4 * (size_t)cnt) && nothing_beyond(jerk, 4 * (size_t)cnt));   // nothing beyond the rows asked for
  }
  // a field call on the same context: phi alone (the stub's phi of point p is -(blocks x w_p))
  void run_field() {
    OK(field(pts.data(), m, skip.data(), nullptr, phi.data()));
    for (int p = 0; p < m; ++p) CHECK(phi[(size_t)p] == (T)(0.0 - (double)nb * (double)p));
  }
  void run_all() {
    run(false, true, true);
    run_field();
    run(true, true, true);
    run(true, true, false);
    run(false, false, true);
    if (m > 2) run(true, true, true, 1, m - 2);
    run_rows();
    if (n > 2) {
      run_rows(1, n - 2);
      run_rows(n - 1, 1, false, true);
      run_rows(n / 4, n / 2 + 1, true, false);   // across both boundaries of three devices
    }
  }
  // the state on the device into pos / vel: what the expectations are computed from after steps
  void refresh() { OK(nbody_sync()); OK(download<T>(pos, vel)); }
};

template <typename T>
static void shapes(int n, int ngpus) {
  for (int m : kShapeM) {
    Case<T> c(n, m);
    c.open(ngpus);
    for_splits(env, {nullptr, "0", "1", "2", "3", "1000"}, [&] { c.run_all(); });
    // after two steps every device's velocities differ from the upload: all N of them must be gathered anew
    if (n >= 3 && m == 257) {
      std::vector<T> before = c.vel;
      OK(step(T(), 0.0078125));
      OK(step(T(), 0.0078125));
      c.refresh();
      CHECK(before != c.vel);
      env.set("2", nullptr);
      c.run_all();
      env.set(nullptr, nullptr);
      c.run_all();
    }
    SHUTDOWN();
  }
}

int main() {
  {
    float one[4] = {0, 0, 0, 0}, a[4] = {5, 5, 5, 5}, j[4] = {5, 5, 5, 5};
    double oned[4] = {0, 0, 0, 0}, ad[4] = {5, 5, 5, 5}, jd[4] = {5, 5, 5, 5};
    CHECK(nbody_jerk(one, one, 1, nullptr, a, j) == NBODY_ERR_NOT_INIT && nbody_jerk_d(oned, oned, 1, nullptr, ad, jd) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_jerk_rows(0, 1, a, j) == NBODY_ERR_NOT_INIT && nbody_jerk_rows_d(0, 1, ad, jd) == NBODY_ERR_NOT_INIT);
    CHECK(a[0] == 5 && j[3] == 5 && ad[0] == 5 && jd[3] == 5);
  }

  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 x 3, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 1000, 2085}, shapes<float>, shapes<double>);

  // ---- the batched path: 69 blocks of per-block sums per query against 1 MB, fp32: 69 x 24 B = 1656 B, batches of 512 queries; a
  // ---- window of rows across the devices' boundary 23333 | 23334 ----
  for_device_counts([](int ngpus) {
    Case<float> c(70000, 5000);
    c.open(ngpus);
    for (const char* split : {(const char*)nullptr, "7", "69"}) {
      env.set(split, "1");
      c.run(true, true, true);
      c.run(false, false, true, 100, 4000);
      c.run_rows(20000, 5000);
    }
    env.set(nullptr, "0");    // not one workgroup's queries fit: no split
    c.run(true, true, true);
    env.set("5", "0");
    c.run_rows(23000, 700, false, true);
    c.run_field();
    SHUTDOWN();
  });
  {
    Case<double> c(70000, 1000);   // 69 x 48 B = 3312 B per query: batches of 256
    c.open(1);
    env.set(nullptr, "1");
    c.run(true, true, true);
    c.run_rows(100, 1000);
    SHUTDOWN();
  }
  env.set(nullptr, nullptr);

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(2085, 300);
    c.open(three_devices() ? 3 : 1);
    float *pts = c.pts.data(), *pv = c.pvel.data(), *a = c.acc.data(), *j = c.jerk.data();
    mark(c.acc); mark(c.jerk);
    CHECK(nbody_jerk(nullptr, pv, 300, nullptr, a, j) == NBODY_ERR_ARG);
    CHECK(nbody_jerk(pts, nullptr, 300, nullptr, a, j) == NBODY_ERR_ARG);
    CHECK(nbody_jerk(pts, pv, 0, nullptr, a, j) == NBODY_ERR_ARG);
    CHECK(nbody_jerk(pts, pv, -1, nullptr, a, j) == NBODY_ERR_ARG);
    CHECK(nbody_jerk(pts, pv, 300, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    for (int bad : refused_skips(2085)) CHECK(nbody_jerk(pts, pv, 300, c.skip_with(299, bad).data(), a, j) == NBODY_ERR_ARG);
    CHECK(nbody_jerk_rows(0, 300, nullptr, nullptr) == NBODY_ERR_ARG);
    for (const Window& w : refused_windows(2085, 300)) CHECK(nbody_jerk_rows(w.first, w.count, a, j) == NBODY_ERR_ARG);
    CHECK(nbody_jerk_rows(2082, 4, a, j) == NBODY_ERR_ARG && nbody_jerk_rows(0, 2086, a, j) == NBODY_ERR_ARG);
    CHECK(nothing_beyond(c.acc, 0) && nothing_beyond(c.jerk, 0));
    std::vector<int> edge = c.skip;
    edge[0] = 2084; edge[299] = 0;
    OK(nbody_jerk(pts, pv, 300, edge.data(), nullptr, j));
    CHECK(nothing_beyond(c.acc, 0));
    std::vector<double> pd(1200, 0.0), ad(1200, 5.0), jd(1200, 5.0);
    CHECK(nbody_jerk_d(pd.data(), pd.data(), 300, nullptr, ad.data(), jd.data()) == NBODY_ERR_STATE && ad[0] == 5.0 && jd[1199] == 5.0);
    CHECK(nbody_jerk_rows_d(0, 300, ad.data(), jd.data()) == NBODY_ERR_STATE && ad[0] == 5.0 && jd[1199] == 5.0);
    c.run_all();
    SHUTDOWN();
    Case<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_jerk(pts, pv, 10, nullptr, a, j) == NBODY_ERR_STATE && nbody_jerk_rows(0, 10, a, j) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a jerk call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(2085, 700);
    const int gather = ngpus > 1 ? 1 : 0;   // ts_vel, where the velocities have to travel
    env.set("3", nullptr);
    int made = sweep("nbody_jerk split", [&] { c.open(ngpus); },
                     [&] { return nbody_jerk(c.pts.data(), c.pvel.data(), c.m, c.skip.data(), c.acc.data(), c.jerk.data()); }, [&] { c.run(true, true, true); });
    CHECK(made == (6 + gather) * ngpus);   // points, point velocities, skip, accel, jerk, scratch per device
    made = sweep("nbody_jerk_rows split", [&] { c.open(ngpus); }, [&] { return nbody_jerk_rows(0, c.n, c.acc.data(), c.jerk.data()); }, [&] { c.run_rows(); });
    CHECK(made == (3 + gather) * ngpus);   // accel, jerk, scratch: the rows are read where they lie
    env.set("1", nullptr);
    made = sweep("nbody_jerk", [&] { c.open(ngpus); }, [&] { return nbody_jerk(c.pts.data(), c.pvel.data(), c.m, nullptr, nullptr, c.jerk.data()); },
                 [&] { c.run(false, false, true); });
    CHECK(made == (3 + gather) * ngpus);   // points, point velocities, jerk
    made = sweep("nbody_jerk_rows", [&] { c.open(ngpus); }, [&] { return nbody_jerk_rows(600, 900, c.acc.data(), nullptr); }, [&] { c.run_rows(600, 900, true, false); });
    CHECK(made == (1 + gather) * ngpus);   // accel
  });
  env.set(nullptr, nullptr);
  field_env.set(nullptr, nullptr);
  printf("jerk_sanity ok\n");
  return 0;
}
