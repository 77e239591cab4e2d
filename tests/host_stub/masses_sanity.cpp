// masses_sanity.cpp — TEST INFRASTRUCTURE (tests/test_masses_host_sanitizers.py): drives NBODY_OPT_MASSES through the library's host
// code (context.cpp, comm.cpp, mailbox.cpp, energy.cpp, point_sums.cpp, timescale.cpp, pair_energy.cpp) against masses_stub.cpp (hip_stub.cpp
// with stand-ins that echo the flag of both argument blocks), timescale_stub.cpp and pair_energy_stub.cpp under AddressSanitizer + UBSan.
// What it checks is the host's logic: the option's values and read-back, that setting it creates nothing, that a fresh context starts
// with 0, the flag in EnergyArgs (nbody_energy, nbody_potential_rows) and in PointSumsArgs (field, tidal, jerk at points and at rows;
// unsplit and split, so the launch and its combine see one flag), a switch of the option between calls on one context, one and
// three stub devices, both precisions, every refusal of §"NBODY_OPT_MASSES" in include/nbody.h — NBODY_ERR_UNSUPPORTED, nothing
// created, outputs and state untouched — the same calls working once the option is off, the mailbox's two refusals and the option
// refused while the mailbox is served, and the failure sweep of a weighted call.
#include <string.h>

#define SANITY_NAME "masses_sanity"
#include "sanity_common.hpp"

extern "C" int masses_stub_energy_flag(void);
extern "C" long masses_stub_energy_launches(void);

static const SplitEnv field_env = {"NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB"};
static const SplitEnv tidal_env = {"NBODY_TIDAL_SPLIT", "NBODY_TIDAL_SCRATCH_MB"};
static const SplitEnv jerk_env = {"NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"};

static long long info(int key) { long long v = -1; OK(nbody_get_info(key, &v)); return v; }
static long live() { long s = 0; for (int kind = 0; kind < 6; ++kind) s += hip_stub_live(kind); return s; }

template <typename T> struct Api;
template <> struct Api<float> {
  static int field(const float* p, int m, const int* sk, float* a, float* phi) { return nbody_field(p, m, sk, a, phi); }
  static int tidal(const float* p, int m, const int* sk, float* t) { return nbody_tidal(p, m, sk, t); }
  static int jerk(const float* p, const float* u, int m, const int* sk, float* a, float* j) { return nbody_jerk(p, u, m, sk, a, j); }
  static int jerk_rows(int f, int m, float* a, float* j) { return nbody_jerk_rows(f, m, a, j); }
  static int potential_rows(int f, int m, float* phi) { return nbody_potential_rows(f, m, phi); }
  static int body_force(float* p, float* v, int n) { return bodyForce(p, v, 0.0078125f, n); }
  static int step(int k) { return nbody_step(0.0078125f, k); }
  static int forces(const float* p, float* f, int n) { return nbody_forces(p, f, n); }
  static int forces_rows(int f, int m, float* out) { return nbody_forces_rows(f, m, out); }
  static int step_adaptive(double* t, int* steps) { return nbody_step_adaptive(0.04f, 0.0078125f, 1e-6f, 1.0f, 4, t, steps); }
  static int pair_energy_rows(int f, int m, float* e, int* idx) { return nbody_pair_energy_rows(f, m, e, idx); }
  static int download(std::vector<float>& p, std::vector<float>& v) { BodySystem b = {p.data(), v.data()}; return nbody_download(&b); }
};
template <> struct Api<double> {
  static int field(const double* p, int m, const int* sk, double* a, double* phi) { return nbody_field_d(p, m, sk, a, phi); }
  static int tidal(const double* p, int m, const int* sk, double* t) { return nbody_tidal_d(p, m, sk, t); }
  static int jerk(const double* p, const double* u, int m, const int* sk, double* a, double* j) { return nbody_jerk_d(p, u, m, sk, a, j); }
  static int jerk_rows(int f, int m, double* a, double* j) { return nbody_jerk_rows_d(f, m, a, j); }
  static int potential_rows(int f, int m, double* phi) { return nbody_potential_rows_d(f, m, phi); }
  static int body_force(double* p, double* v, int n) { return bodyForce_d(p, v, 0.0078125, n); }
  static int step(int k) { return nbody_step_d(0.0078125, k); }
  static int forces(const double* p, double* f, int n) { return nbody_forces_d(p, f, n); }
  static int forces_rows(int f, int m, double* out) { return nbody_forces_rows_d(f, m, out); }
  static int step_adaptive(double* t, int* steps) { return nbody_step_adaptive_d(0.04, 0.0078125, 1e-6, 1.0, 4, t, steps); }
  static int pair_energy_rows(int f, int m, double* e, int* idx) { return nbody_pair_energy_rows_d(f, m, e, idx); }
  static int download(std::vector<double>& p, std::vector<double>& v) { BodySystemD b = {p.data(), v.data()}; return nbody_download_d(&b); }
};

template <class V, typename T> static bool all_are(const V& v, size_t count, T value) {
  for (size_t k = 0; k < count; ++k) if (v[k] != value) return false;
  return true;
}

template <typename T>
struct Case : Fixture<T> {
  using Fixture<T>::n; using Fixture<T>::m; using Fixture<T>::pos; using Fixture<T>::vel; using Fixture<T>::pts; using Fixture<T>::skip;
  std::vector<T> pvel, out0, out1, phi, e;
  std::vector<int> idx;
  int rows;
  Case(int n_, int m_) : Fixture<T>(n_, m_), pvel((size_t)m_ * 4, (T)1), rows(std::max(n_, m_)) {
    out0.resize((size_t)rows * 6); out1.resize((size_t)rows * 4); phi.resize((size_t)rows); e.resize((size_t)n_); idx.resize((size_t)n_);
    for (int j = 0; j < n; ++j) this->set(vel, j, (T)(j % 3), (T)1, (T)0, (T)0);
  }
  // every weighted pass with the option as it stands: the stub's echo says which flag the launches carried (split: the combine's value)
  void expect_flag(int flag, bool split) {
    const T want = (T)((split ? 3 : 1) + flag);
    mark(out0); mark(out1);
    OK(Api<T>::field(pts.data(), m, skip.data(), out0.data(), out1.data()));
    CHECK(all_are(out0, 4 * (size_t)m, want) && all_are(out1, (size_t)m, want) && nothing_beyond(out0, 4 * (size_t)m) && nothing_beyond(out1, (size_t)m));
    mark(out0);
    OK(Api<T>::tidal(pts.data(), m, nullptr, out0.data()));
    CHECK(all_are(out0, 6 * (size_t)m, want) && nothing_beyond(out0, 6 * (size_t)m));
    mark(out0); mark(out1);
    OK(Api<T>::jerk(pts.data(), pvel.data(), m, skip.data(), out0.data(), out1.data()));
    CHECK(all_are(out0, 4 * (size_t)m, want) && all_are(out1, 4 * (size_t)m, want) && nothing_beyond(out0, 4 * (size_t)m));
    mark(out0); mark(out1);
    OK(Api<T>::jerk_rows(0, n, out0.data(), out1.data()));
    CHECK(all_are(out0, 4 * (size_t)n, want) && all_are(out1, 4 * (size_t)n, want) && nothing_beyond(out1, 4 * (size_t)n));
    double tot[NBODY_ENERGY_WORDS];
    long before = masses_stub_energy_launches();
    OK(nbody_energy(tot));
    CHECK(masses_stub_energy_launches() > before && masses_stub_energy_flag() == flag);
    before = masses_stub_energy_launches();
    OK(Api<T>::potential_rows(0, n, phi.data()));
    CHECK(masses_stub_energy_launches() > before && masses_stub_energy_flag() == flag);
    CHECK(info(NBODY_INFO_MASSES) == flag);
  }
  // the option on: every unit-mass entry point refuses, creates nothing, writes nothing, and the state on the device stays
  void expect_refusals() {
    std::vector<T> p0((size_t)n * 4), v0((size_t)n * 4), p1 = p0, v1 = v0, hp = pos, hv = vel;
    OK(nbody_sync()); OK(Api<T>::download(p0, v0));
    const long long steps = info(NBODY_INFO_STEPS_DONE);
    const long held = live();
    double t = kMark; int taken = kMark, found = kMark;
    std::vector<double> el((size_t)n * NBODY_BINARY_WORDS, (double)kMark);
    mark(out0); mark(e); mark(idx);
    CHECK(Api<T>::body_force(hp.data(), hv.data(), n) == NBODY_ERR_UNSUPPORTED);
    CHECK(Api<T>::step(1) == NBODY_ERR_UNSUPPORTED && Api<T>::step(70) == NBODY_ERR_UNSUPPORTED);
    CHECK(Api<T>::forces(hp.data(), out0.data(), n) == NBODY_ERR_UNSUPPORTED);
    CHECK(Api<T>::forces_rows(0, n, out0.data()) == NBODY_ERR_UNSUPPORTED);
    CHECK(Api<T>::step_adaptive(&t, &taken) == NBODY_ERR_UNSUPPORTED);
    CHECK(Api<T>::pair_energy_rows(0, n, e.data(), idx.data()) == NBODY_ERR_UNSUPPORTED);
    CHECK(nbody_binaries(0.0, n, &found, idx.data(), idx.data(), el.data()) == NBODY_ERR_UNSUPPORTED);
    CHECK(live() == held && info(NBODY_INFO_STEPS_DONE) == steps);
    CHECK(nothing_beyond(out0, 0) && nothing_beyond(e, 0) && nothing_beyond(idx, 0) && nothing_beyond(el, 0));
    CHECK(t == kMark && taken == kMark && found == kMark && hp == pos && hv == vel);
    OK(nbody_sync()); OK(Api<T>::download(p1, v1));
    CHECK(p1 == p0 && v1 == v0);
  }
  // the option off: the same calls work
  void expect_work() {
    std::vector<T> hp = pos, hv = vel;
    double t = 0.0; int taken = 0, found = 0;
    std::vector<double> el((size_t)n * NBODY_BINARY_WORDS);
    OK(Api<T>::forces_rows(0, n, out0.data()));
    OK(Api<T>::pair_energy_rows(0, n, e.data(), idx.data()));
    OK(nbody_binaries(0.0, n, &found, idx.data(), idx.data(), el.data()));
    OK(Api<T>::step(1)); OK(Api<T>::step(70)); OK(nbody_sync());
    OK(Api<T>::step_adaptive(&t, &taken));
    OK(Api<T>::forces(hp.data(), out0.data(), n));
    OK(Api<T>::body_force(hp.data(), hv.data(), n));
    OK(upload<T>(pos, vel));
  }
};

template <typename T>
static void shapes(int n, int ngpus) {
  const std::initializer_list<const SplitEnv*> envs = {&field_env, &tidal_env, &jerk_env};
  for (const SplitEnv* env : envs) env->set("1", nullptr);   // one chunk unless a section says otherwise (the automatic split follows N and m)
  Case<T> c(n, 700);
  c.open(ngpus);
  CHECK(info(NBODY_INFO_MASSES) == 0);            // a fresh context starts with unit masses
  const long held = live();
  c.expect_flag(0, false);
  const long after_calls = live();
  OK(nbody_set_option(NBODY_OPT_MASSES, 1));
  CHECK(live() == after_calls && held <= after_calls);   // setting the option creates nothing
  CHECK(nbody_set_option(NBODY_OPT_MASSES, 2) == NBODY_ERR_ARG && nbody_set_option(NBODY_OPT_MASSES, -1) == NBODY_ERR_ARG);
  c.expect_flag(1, false);
  c.expect_refusals();
  if (n >= 2049) {   // three blocks and a forced split: the launch and its combine carry one flag
    for (const SplitEnv* env : envs) env->set("3", nullptr);
    c.expect_flag(1, true);
    OK(nbody_set_option(NBODY_OPT_MASSES, 0));   // a switch between calls on one context
    c.expect_flag(0, true);
    OK(nbody_set_option(NBODY_OPT_MASSES, 1));
    for (const SplitEnv* env : envs) env->set(nullptr, "0");   // (not one workgroup's queries fit: no split)
    c.expect_flag(1, false);
    for (const SplitEnv* env : envs) env->set("1", nullptr);
  }
  OK(nbody_set_option(NBODY_OPT_MASSES, 0));
  c.expect_flag(0, false);
  c.expect_work();
  OK(nbody_set_option(NBODY_OPT_MASSES, 1));     // after steps and a captured graph: still a refusal, still nothing touched
  c.expect_refusals();
  c.expect_flag(1, false);
  SHUTDOWN();
  OK(nbody_init(n, ngpus, sizeof(T) == 8, 0));    // the option does not outlive its context
  CHECK(info(NBODY_INFO_MASSES) == 0);
  SHUTDOWN();
  for (const SplitEnv* env : envs) env->set(nullptr, nullptr);
}

int main() {
  {
    long long v = 5;
    CHECK(nbody_get_info(NBODY_INFO_MASSES, &v) == NBODY_ERR_NOT_INIT && v == 5);
    CHECK(nbody_set_option(NBODY_OPT_MASSES, 3) == NBODY_ERR_ARG);
  }
  for_sizes({1, 1000, 2085}, shapes<float>, shapes<double>);
  for_device_counts([](int ngpus) { shapes<float>(3000, ngpus); });

  // ---- the mailbox: a request is the reference's force pass ----
  {
    OK(nbody_init(500, 1, 0, 0));
    OK(nbody_set_option(NBODY_OPT_MASSES, 1));
    SHUTDOWN();
    OK(nbody_mailbox_open(1024, 0));
    CHECK(info(NBODY_INFO_MASSES) == 0);         // nbody_mailbox_open opens a fresh context
    void *ram_a = nullptr, *ram_b = nullptr; int cap = 0;
    OK(nbody_mailbox_rams(&ram_a, &ram_b, &cap));
    OK(nbody_set_option(NBODY_OPT_MASSES, 1));
    const long held = live();
    std::vector<unsigned char> a0((unsigned char*)ram_a, (unsigned char*)ram_a + 16 * (size_t)(cap + 1));
    CHECK(nbody_mailbox_run(ram_a, ram_b, 0) == NBODY_ERR_UNSUPPORTED);
    CHECK(nbody_mailbox_serve(1, 300000) == NBODY_ERR_UNSUPPORTED && info(NBODY_INFO_MAILBOX_SERVING) == 0);
    CHECK(live() == held && memcmp(a0.data(), ram_a, a0.size()) == 0);
    OK(nbody_mailbox_serve(0, 0));               // stopping what does not run stays legal
    OK(nbody_set_option(NBODY_OPT_MASSES, 0));
    OK(nbody_mailbox_serve(1, 300000));
    CHECK(nbody_set_option(NBODY_OPT_MASSES, 1) == NBODY_ERR_STATE && info(NBODY_INFO_MASSES) == 0);   // like every other option
    OK(nbody_mailbox_serve(0, 0));
    OK(nbody_set_option(NBODY_OPT_MASSES, 1));
    CHECK(info(NBODY_INFO_MASSES) == 1);
    SHUTDOWN();
  }

  // ---- the failure paths of a weighted call ----
  for_device_counts([](int ngpus) {
    Case<float> c(2085, 700);
    field_env.set("3", nullptr);
    sweep("nbody_field with masses", [&] { c.open(ngpus); OK(nbody_set_option(NBODY_OPT_MASSES, 1)); },
          [&] { return nbody_field(c.pts.data(), c.m, c.skip.data(), c.out0.data(), c.out1.data()); },
          [&] { CHECK(all_are(c.out0, 4 * (size_t)c.m, 4.0f) && all_are(c.out1, (size_t)c.m, 4.0f)); });
    field_env.set(nullptr, nullptr);
    sweep("nbody_energy with masses", [&] { c.open(ngpus); OK(nbody_set_option(NBODY_OPT_MASSES, 1)); },
          [&] { double tot[NBODY_ENERGY_WORDS]; return nbody_energy(tot); }, [&] { CHECK(masses_stub_energy_flag() == 1); });
  });
  printf("masses_sanity ok\n");
  return 0;
}
