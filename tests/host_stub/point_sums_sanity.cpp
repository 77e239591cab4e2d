// point_sums_sanity.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): drives nbody_field(_d) or nbody_tidal(_d) — the pass its
// argument names — of the library's host code (point_sums.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp) against
// tests/host_stub/hip_stub.cpp and point_sums_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's logic: the division
// of the points over the devices, the upload and copy-back offsets of each output, the choice of the source split, the scratch size and
// the batches, the argument checks, nbody_field calls between tidal calls (the two passes share their buffers), lifetimes at shutdown
// and the failure paths.  point_sums_stub.cpp states the values expected here.
#include <string.h>

#define SANITY_NAME "point_sums_sanity"
#include "sanity_common.hpp"

static SplitEnv env;   // the two variables of the pass under test: main sets them

static int field(const float* p, int m, const int* sk, float* a, float* phi) { return nbody_field(p, m, sk, a, phi); }
static int field(const double* p, int m, const int* sk, double* a, double* phi) { return nbody_field_d(p, m, sk, a, phi); }
static int tidal(const float* p, int m, const int* sk, float* t) { return nbody_tidal(p, m, sk, t); }
static int tidal(const double* p, int m, const int* sk, double* t) { return nbody_tidal_d(p, m, sk, t); }

// what both passes' cases are made of: the shared fixture's points and skip indices, this driver's own bodies (x = j mod 13, in which
// the stub's sums have a closed form) and the stub's sums at a point
template <typename T>
struct Points : Fixture<T> {
  using Fixture<T>::n; using Fixture<T>::skip;
  int nb;
  Points(int n_, int m_) : Fixture<T>(n_, m_), nb(stub::blocks_of(n_)) {
    for (int j = 0; j < n; ++j) this->set(this->pos, j, (T)(j % 13), (T)(j % 7), (T)1, (T)1);
  }
  // the level-2 sums Q0, Q1, Q2 of point p (Q3 = nb p, Q4 = nb (nb - 1) / 2, Q5 = nb, Q6 = 3 nb)
  void sums(int p, bool with_skip, double q[3]) const {
    q[0] = q[1] = 0.0;
    for (int b = 0; b < nb; ++b) { q[0] += (double)(T)((T)((b * stub::kBlock) % 13) - (T)(p % 17)); q[1] += (double)(T)((T)(p % 5) + (T)b); }
    q[2] = (double)nb * (double)(with_skip ? skip[(size_t)p] : -1) + (double)((n - 1) % 13);
  }
};

template <typename T>
struct FieldCase : Points<T> {
  std::vector<T> acc, phi;
  FieldCase(int n_, int m_) : Points<T>(n_, m_), acc((size_t)m_ * 4), phi((size_t)m_) {}
  // points [p0, p0 + cnt) of the case, with or without skip and either output
  void run(bool with_skip, bool want_acc, bool want_phi, int p0 = 0, int cnt = -1) {
    const int m = this->m;
    if (cnt < 0) cnt = m - p0;
    const T unwritten = (T)kMark;
    mark(acc); mark(phi);
    OK(field(this->pts.data() + 4 * (size_t)p0, cnt, with_skip ? this->skip.data() + p0 : nullptr, want_acc ? acc.data() : nullptr, want_phi ? phi.data() : nullptr));
    for (int k = 0; k < cnt; ++k) {
      const int p = p0 + k;
      double q[3];
      this->sums(p, with_skip, q);
      if (want_acc) CHECK(acc[4 * (size_t)k] == (T)q[0] && acc[4 * (size_t)k + 1] == (T)q[1] && acc[4 * (size_t)k + 2] == (T)q[2] && acc[4 * (size_t)k + 3] == (T)0);
      else CHECK(acc[4 * (size_t)k] == unwritten);
      if (want_phi) CHECK(phi[(size_t)k] == (T)(0.0 - (double)this->nb * (double)p));
      else CHECK(phi[(size_t)k] == unwritten);
    }
    CHECK(nothing_beyond(acc, 4 * (size_t)cnt) && nothing_beyond(phi, (size_t)cnt));   // nothing beyond the points asked for
  }
  void run_all() {
    run(false, true, true);
    run(true, true, true);
    run(true, true, false);
    run(false, false, true);
    if (this->m > 2) run(true, true, true, 1, this->m - 2);
  }
};

template <typename T>
struct TidalCase : Points<T> {
  std::vector<T> out, phi;
  TidalCase(int n_, int m_) : Points<T>(n_, m_), out((size_t)m_ * 6), phi((size_t)m_) {}
  // points [p0, p0 + cnt) of the case, with or without skip
  void run(bool with_skip, int p0 = 0, int cnt = -1) {
    if (cnt < 0) cnt = this->m - p0;
    mark(out);
    OK(tidal(this->pts.data() + 4 * (size_t)p0, cnt, with_skip ? this->skip.data() + p0 : nullptr, out.data()));
    const int nb = this->nb;
    const double s3 = 3.0 * (double)nb;
    for (int k = 0; k < cnt; ++k) {
      const int p = p0 + k;
      double q[3];
      this->sums(p, with_skip, q);
      const T* t = out.data() + 6 * (size_t)k;
      CHECK(t[0] == (T)(q[0] - s3) && t[1] == (T)(q[1] - s3) && t[2] == (T)(q[2] - s3));
      CHECK(t[3] == (T)((double)nb * (double)p) && t[4] == (T)((double)nb * (double)(nb - 1) / 2.0) && t[5] == (T)nb);
    }
    CHECK(nothing_beyond(out, 6 * (size_t)cnt));   // nothing beyond the points asked for
  }
  // a field call on the same context: phi alone
  void run_field() {
    OK(field(this->pts.data(), this->m, this->skip.data(), nullptr, phi.data()));
    for (int p = 0; p < this->m; ++p) CHECK(phi[(size_t)p] == (T)(0.0 - (double)this->nb * (double)p));
  }
  void run_all() {
    run(false);
    run_field();
    run(true);
    if (this->m > 2) run(true, 1, this->m - 2);
  }
};

template <class C>
static void shapes(int n, int ngpus) {
  for (int m : kShapeM) {
    C c(n, m);
    c.open(ngpus);
    for_splits(env, {nullptr, "0", "1", "2", "3", "1000"}, [&] { c.run_all(); });
    SHUTDOWN();
  }
}

// what the two passes are driven through alike (C: FieldCase or TidalCase)
template <template <typename> class C>
static void shapes_and_batches() {
  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 + 695 + 695, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 1000, 2085}, shapes<C<float>>, shapes<C<double>>);

  // ---- the batched path: 69 blocks of per-block sums per point against 1 MB, fp32: field 69 x 16 B = 1104 B, batches of 768 points;
  // ---- tidal 69 x 28 B = 1932 B, batches of 512 ----
  for_device_counts([](int ngpus) {
    C<float> c(70000, 5000);
    c.open(ngpus);
    for (const char* split : {(const char*)nullptr, "7", "69"}) {
      env.set(split, "1");
      c.run_all();
    }
    env.set(nullptr, "0");    // not one workgroup's points fit: no split
    c.run_all();
    env.set("5", "0");
    c.run_all();
    SHUTDOWN();
  });
  {
    C<double> c(70000, 1000);   // field 2208 B per point, tidal 3864 B: batches of 256
    c.open(1);
    env.set(nullptr, "1");
    c.run_all();
    SHUTDOWN();
  }
  env.set(nullptr, nullptr);
}

static void field_main() {
  float one[4] = {0, 0, 0, 0}, out[4] = {5, 5, 5, 5}, ph[1] = {5};
  double oned[4] = {0, 0, 0, 0}, outd[4] = {5, 5, 5, 5}, phd[1] = {5};
  CHECK(nbody_field(one, 1, nullptr, out, ph) == NBODY_ERR_NOT_INIT && nbody_field_d(oned, 1, nullptr, outd, phd) == NBODY_ERR_NOT_INIT);

  shapes_and_batches<FieldCase>();

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    FieldCase<float> c(2085, 300);
    c.open(three_devices() ? 3 : 1);
    float* pts = c.pts.data();
    mark(c.acc); mark(c.phi);
    CHECK(nbody_field(nullptr, 300, nullptr, c.acc.data(), c.phi.data()) == NBODY_ERR_ARG);
    CHECK(nbody_field(pts, 0, nullptr, c.acc.data(), c.phi.data()) == NBODY_ERR_ARG);
    CHECK(nbody_field(pts, -1, nullptr, c.acc.data(), c.phi.data()) == NBODY_ERR_ARG);
    CHECK(nbody_field(pts, 300, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    for (int bad : refused_skips(2085)) CHECK(nbody_field(pts, 300, c.skip_with(299, bad).data(), c.acc.data(), c.phi.data()) == NBODY_ERR_ARG);
    std::vector<int> edge = c.skip;
    edge[0] = 2084; edge[299] = 0;
    OK(nbody_field(pts, 300, edge.data(), nullptr, c.phi.data()));
    CHECK(nothing_beyond(c.acc, 0));
    std::vector<double> pd(1200, 0.0), ad(1200, 5.0), fd(300, 5.0);
    CHECK(nbody_field_d(pd.data(), 300, nullptr, ad.data(), fd.data()) == NBODY_ERR_STATE && ad[0] == 5.0 && fd[299] == 5.0);
    c.run_all();
    SHUTDOWN();
    FieldCase<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_field(pts, 10, nullptr, c.acc.data(), c.phi.data()) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a field call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    FieldCase<float> c(2085, 700);
    env.set("3", nullptr);
    int made = sweep("nbody_field split", [&] { c.open(ngpus); }, [&] { return nbody_field(c.pts.data(), c.m, c.skip.data(), c.acc.data(), c.phi.data()); },
                     [&] { c.run(true, true, true); });
    CHECK(made == 5 * ngpus);   // points, skip, accel, phi, scratch per device
    env.set("1", nullptr);
    made = sweep("nbody_field", [&] { c.open(ngpus); }, [&] { return nbody_field(c.pts.data(), c.m, nullptr, nullptr, c.phi.data()); },
                 [&] { c.run(false, false, true); });
    CHECK(made == 2 * ngpus);   // points, phi
  });
  env.set(nullptr, nullptr);
}

static void tidal_main() {
  float one[4] = {0, 0, 0, 0}, out[6] = {5, 5, 5, 5, 5, 5};
  double oned[4] = {0, 0, 0, 0}, outd[6] = {5, 5, 5, 5, 5, 5};
  CHECK(nbody_tidal(one, 1, nullptr, out) == NBODY_ERR_NOT_INIT && nbody_tidal_d(oned, 1, nullptr, outd) == NBODY_ERR_NOT_INIT);
  CHECK(out[0] == 5 && outd[5] == 5);

  shapes_and_batches<TidalCase>();

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    TidalCase<float> c(2085, 300);
    c.open(three_devices() ? 3 : 1);
    float* pts = c.pts.data();
    mark(c.out);
    CHECK(nbody_tidal(nullptr, 300, nullptr, c.out.data()) == NBODY_ERR_ARG);
    CHECK(nbody_tidal(pts, 300, nullptr, nullptr) == NBODY_ERR_ARG);
    CHECK(nbody_tidal(pts, 0, nullptr, c.out.data()) == NBODY_ERR_ARG);
    CHECK(nbody_tidal(pts, -1, nullptr, c.out.data()) == NBODY_ERR_ARG);
    for (int bad : refused_skips(2085)) CHECK(nbody_tidal(pts, 300, c.skip_with(299, bad).data(), c.out.data()) == NBODY_ERR_ARG);
    CHECK(nothing_beyond(c.out, 0));
    std::vector<int> edge = c.skip;
    edge[0] = 2084; edge[299] = 0;
    OK(nbody_tidal(pts, 300, edge.data(), c.out.data()));
    std::vector<double> pd(1200, 0.0), td(1800, 5.0);
    CHECK(nbody_tidal_d(pd.data(), 300, nullptr, td.data()) == NBODY_ERR_STATE && td[0] == 5.0 && td[1799] == 5.0);
    c.run_all();
    SHUTDOWN();
    TidalCase<double> d(1000, 10);
    d.open(1);
    CHECK(nbody_tidal(pts, 10, nullptr, c.out.data()) == NBODY_ERR_STATE);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a tidal call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    TidalCase<float> c(2085, 700);
    env.set("3", nullptr);
    int made = sweep("nbody_tidal split", [&] { c.open(ngpus); }, [&] { return nbody_tidal(c.pts.data(), c.m, c.skip.data(), c.out.data()); },
                     [&] { c.run(true); });
    CHECK(made == 4 * ngpus);   // points, skip, tensor, scratch per device
    env.set("1", nullptr);
    made = sweep("nbody_tidal", [&] { c.open(ngpus); }, [&] { return nbody_tidal(c.pts.data(), c.m, nullptr, c.out.data()); },
                 [&] { c.run(false); });
    CHECK(made == 2 * ngpus);   // points, tensor
  });
  env.set(nullptr, nullptr);
}

int main(int argc, char** argv) {
  const std::string pass = argc > 1 ? argv[1] : "";
  CHECK(pass == "field" || pass == "tidal");
  env = pass == "field" ? SplitEnv{"NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB"} : SplitEnv{"NBODY_TIDAL_SPLIT", "NBODY_TIDAL_SCRATCH_MB"};
  if (pass == "field") field_main(); else tidal_main();
  printf("point_sums_sanity %s ok\n", pass.c_str());
  return 0;
}
