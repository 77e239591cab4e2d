// pair_energy_sanity.cpp — TEST INFRASTRUCTURE (tests/test_pair_energy_host.py): drives nbody_pair_energy_rows(_d) and nbody_binaries of
// the library's host code (pair_energy.cpp beside context.cpp, comm.cpp, mailbox.cpp and energy.cpp) against tests/host_stub/hip_stub.cpp
// and pair_energy_stub.cpp under AddressSanitizer + UBSan.  What it checks is the host's logic: the rows of a window over the devices,
// the copy-back offsets of the two outputs, the gather of all N velocities to every device, the choice of the source split, the scratch
// size and the batches, the all-rows walk of nbody_binaries in contiguous ranges over the devices, the mutual test, e_max, max_pairs and
// the members the elements are computed from, the argument checks, lifetimes at shutdown and the failure paths.  pair_energy_stub.cpp
// states the values expected here.
// It covers one and three stub devices with ragged slices, windows of rows across the devices, the source split forced and automatic,
// the batched path under a small scratch bound, the gather of all N velocities on three devices after steps have changed them, every
// NBODY_ERR_ARG case and the failure sweep of sanity_common.hpp.
#include <math.h>
#include <string.h>

#include <limits>

#define SANITY_NAME "pair_energy_sanity"
#include "sanity_common.hpp"

static const SplitEnv env = {"NBODY_PAIR_ENERGY_SPLIT", "NBODY_PAIR_ENERGY_SCRATCH_MB"};

static int rows(int f, int m, float* e, int* i) { return nbody_pair_energy_rows(f, m, e, i); }
static int rows(int f, int m, double* e, int* i) { return nbody_pair_energy_rows_d(f, m, e, i); }
static int step(float, double dt) { return nbody_step((float)dt, 1); }
static int step(double, double dt) { return nbody_step_d(dt, 1); }
template <typename T> int download(std::vector<T>& pos, std::vector<T>& vel);
template <> int download<float>(std::vector<float>& pos, std::vector<float>& vel) { BodySystem b = {pos.data(), vel.data()}; return nbody_download(&b); }
template <> int download<double>(std::vector<double>& pos, std::vector<double>& vel) { BodySystemD b = {pos.data(), vel.data()}; return nbody_download_d(&b); }

// equal, or both NaN, or within 1e-12 relative (the driver's compiler may round an expression otherwise than the library's)
static bool close_to(double got, double want) {
  if (got != got || want != want) return got != got && want != want;
  if (got == want) return true;
  return fabs(got - want) <= 1e-12 * fabs(want);
}

// small integers everywhere: every value of pair_energy_stub.cpp is exact in either precision.  w steers the stub rule to the body
// beside a body (j ^ 1): in a one-block system every pair (2k, 2k + 1) is mutual
template <typename T>
struct Case : System<T> {
  using System<T>::n; using System<T>::pos; using System<T>::vel;
  std::vector<T> e;
  std::vector<int> idx;
  explicit Case(int n_) : System<T>(n_), e((size_t)n_), idx((size_t)n_) {
    for (int j = 0; j < n; ++j) {
      this->set(pos, j, (T)(j % 13), (T)(j % 7), (T)1, (T)(j ^ 1));
      vel[4 * (size_t)j] = (T)((j * 7) % 11);
      vel[4 * (size_t)j + 1] = (T)(j % 3);
    }
  }
  // what the stub makes of row i of the state in pos / vel
  void expect(int i, T* q, int* ix) const {
    *q = std::numeric_limits<T>::infinity(); *ix = -1;
    for (int b = 0; b < stub::blocks_of(n); ++b) {
      const int j = stub::candidate(n, pos[4 * (size_t)i + 3], b).j;
      if (j == i) continue;
      const T c = stub::absdiff(pos[4 * (size_t)j], pos[4 * (size_t)i]) - stub::absdiff(vel[4 * (size_t)j], vel[4 * (size_t)i]) - (T)3;
      if (c < *q) { *q = c; *ix = j; }
    }
  }
  // rows [first, first + cnt) with the outputs in `which` (bit 0 e, 1 idx)
  void run(int first = 0, int cnt = -1, int which = 3) {
    if (cnt < 0) cnt = n - first;
    mark(e); mark(idx);
    OK(rows(first, cnt, which & 1 ? e.data() : nullptr, which & 2 ? idx.data() : nullptr));
    for (int k = 0; k < cnt; ++k) {
      T q;
      int ix;
      expect(first + k, &q, &ix);
      CHECK(e[(size_t)k] == (which & 1 ? q : (T)kMark));
      CHECK(idx[(size_t)k] == (which & 2 ? ix : kMark));
    }
    CHECK(nothing_beyond(e, (size_t)cnt) && nothing_beyond(idx, (size_t)cnt));   // nothing beyond the rows asked for
  }
  // {E, a, ecc, period} of (i, j) from the state in pos / vel: include/nbody.h's operations
  void elements(int i, int j, double* out) const {
    const T *ri = &pos[4 * (size_t)i], *rj = &pos[4 * (size_t)j], *vi = &vel[4 * (size_t)i], *vj = &vel[4 * (size_t)j];
    const double dx = (double)rj[0] - (double)ri[0], dy = (double)rj[1] - (double)ri[1], dz = (double)rj[2] - (double)ri[2];
    const double ux = (double)vj[0] - (double)vi[0], uy = (double)vj[1] - (double)vi[1], uz = (double)vj[2] - (double)vi[2];
    const unsigned eps_bits = 0x3089705Fu;
    float eps;
    memcpy(&eps, &eps_bits, sizeof(eps));
    const double r = sqrt(((dx * dx + dy * dy) + dz * dz) + (double)eps), v2 = (ux * ux + uy * uy) + uz * uz;
    const double E = 0.5 * v2 - 2.0 / r, a = -1.0 / E;
    const double cx = dy * uz - dz * uy, cy = dz * ux - dx * uz, cz = dx * uy - dy * ux;
    const double k = 1.0 + (0.5 * E) * ((cx * cx + cy * cy) + cz * cz);
    out[0] = E; out[1] = a; out[2] = sqrt(k > 0.0 ? k : 0.0); out[3] = 3.14159265358979323846 * sqrt(((2.0 * a) * a) * a);
  }
  // nbody_binaries below e_max with room for max_pairs against the mutual test over expect(); returns the number found
  int run_binaries(double e_max, int max_pairs) {
    std::vector<T> q((size_t)n);
    std::vector<int> ix((size_t)n), wi, wj;
    for (int i = 0; i < n; ++i) expect(i, &q[(size_t)i], &ix[(size_t)i]);
    for (int i = 0; i < n; ++i) {
      const int j = ix[(size_t)i];
      if (j > i && ix[(size_t)j] == i && (double)q[(size_t)i] < e_max) { wi.push_back(i); wj.push_back(j); }
    }
    const size_t room = (size_t)max_pairs + 2;   // two marked slots beyond what may be written
    std::vector<int> gi(room), gj(room);
    std::vector<double> el(room * NBODY_BINARY_WORDS);
    mark(gi); mark(gj); mark(el);
    int found = kMark;
    OK(nbody_binaries(e_max, max_pairs, &found, max_pairs ? gi.data() : nullptr, max_pairs ? gj.data() : nullptr, max_pairs ? el.data() : nullptr));
    CHECK(found == (int)wi.size());
    const size_t listed = std::min((size_t)max_pairs, wi.size());
    for (size_t k = 0; k < listed; ++k) {
      double want[NBODY_BINARY_WORDS];
      CHECK(gi[k] == wi[k] && gj[k] == wj[k]);
      elements(wi[k], wj[k], want);
      for (int c = 0; c < NBODY_BINARY_WORDS; ++c) CHECK(close_to(el[NBODY_BINARY_WORDS * k + (size_t)c], want[c]));
    }
    CHECK(nothing_beyond(gi, listed) && nothing_beyond(gj, listed) && nothing_beyond(el, listed * NBODY_BINARY_WORDS));
    return found;
  }
  void run_system() {
    const int all = run_binaries(0.0, n);
    CHECK(run_binaries(0.0, 0) == all);                   // max_pairs == 0 counts, the arrays may be NULL
    if (all > 1) CHECK(run_binaries(0.0, 1) == all);      // *n_pairs may exceed max_pairs: the lowest i is listed
    const int some = run_binaries(-6.0, n);               // the stub's e reaches -13
    CHECK(some <= all);
    CHECK(run_binaries(-std::numeric_limits<double>::infinity(), n) == 0);
  }
  void run_all() {
    run();
    run_system();
    if (n > 2) { run(1, n - 2); run(n - 1, 1, 2); run(0, n, 1); run(0, n / 2 + 1, 2); }
  }
  // the state on the device into pos / vel: what the expectations are computed from after steps
  void refresh() { OK(nbody_sync()); OK(download<T>(pos, vel)); }
};

template <typename T>
static void shapes(int n, int ngpus) {
  Case<T> c(n);
  c.open(ngpus);
  for_splits(env, {nullptr, "0", "1", "2", "3", "1000"}, [&] { c.run_all(); });
  if (n == 1000) {   // one block: every pair (2k, 2k + 1) is mutual, and those with e < 0 are listed
    CHECK(c.run_binaries(0.0, n) > 100);
    CHECK(c.run_binaries(-6.0, n) > 0 && c.run_binaries(-6.0, n) < c.run_binaries(0.0, n));
  }
  // after two steps every device's velocities differ from the upload: all N of them must be gathered anew
  if (n >= 3) {
    OK(step(T(), 0.0078125));
    OK(step(T(), 0.0078125));
    c.refresh();
    // (the state is no longer small integers: the stub's differences round, identically here and there; w is untouched by a step)
    env.set("2", nullptr);
    c.run_all();
    env.set(nullptr, nullptr);
    c.run_all();
  }
  SHUTDOWN();
}

int main() {
  {
    float e[4] = {5, 5, 5, 5};
    double ed[8] = {5, 5, 5, 5, 5, 5, 5, 5};
    int ix[4] = {5, 5, 5, 5}, found = 5;
    CHECK(nbody_pair_energy_rows(0, 4, e, ix) == NBODY_ERR_NOT_INIT && nbody_pair_energy_rows_d(0, 4, ed, ix) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_binaries(0.0, 2, &found, ix, ix + 2, ed) == NBODY_ERR_NOT_INIT && nbody_binaries(0.0, 0, &found, nullptr, nullptr, nullptr) == NBODY_ERR_NOT_INIT);
    CHECK(e[0] == 5 && ed[1] == 5 && ix[0] == 5 && ix[2] == 5 && found == 5);
  }

  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 x 3, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 2, 1000, 2085}, shapes<float>, shapes<double>);

  // ---- the batched path: 7 chunks x 8 B = 56 B per row against 0.05 MB = 52428 B: batches of 768 rows (fp32); a window across the
  //      devices' boundary 23333 | 23334 ----
  for_device_counts([](int ngpus) {
    Case<float> c(70000);
    c.open(ngpus);
    for (const char* split : {"7", "69"}) {
      env.set(split, "0.05");
      c.run(20000, 5000);
      c.run(23000, 700, 1);
    }
    env.set(nullptr, "0.05");
    c.run(20000, 5000);
    env.set("5", "0");    // not one workgroup's rows fit: no split
    c.run(23000, 700);
    env.set("3", "0.05");
    c.run_binaries(0.0, 100);
    SHUTDOWN();
  });
  {
    Case<double> c(70000);   // 7 chunks x 12 B = 84 B per row: batches of 512
    c.open(1);
    env.set("7", "0.05");
    c.run(100, 1000);
    SHUTDOWN();
  }
  env.set(nullptr, nullptr);

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(2085);
    c.open(three_devices() ? 3 : 1);
    std::vector<float> e(2085, (float)kMark);
    std::vector<int> ix(2085, kMark), jx(2085, kMark);
    std::vector<double> el(2085 * NBODY_BINARY_WORDS, (double)kMark);
    int found = kMark;
    CHECK(nbody_pair_energy_rows(0, 2085, nullptr, nullptr) == NBODY_ERR_ARG);
    // this pass's own windows (a rows form only, no count of 300): not sanity_common.hpp's list
    const int bad_rows[][2] = {{-1, 4}, {0, 0}, {0, -2}, {2082, 4}, {2085, 1}, {0, 2086}, {1 << 30, 1 << 30}};
    for (const auto& r : bad_rows) CHECK(nbody_pair_energy_rows(r[0], r[1], e.data(), ix.data()) == NBODY_ERR_ARG);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double e_max : {nan, 0.5, 1e-300, inf}) CHECK(nbody_binaries(e_max, 10, &found, ix.data(), jx.data(), el.data()) == NBODY_ERR_ARG);
    CHECK(nbody_binaries(0.0, -1, &found, ix.data(), jx.data(), el.data()) == NBODY_ERR_ARG);
    CHECK(nbody_binaries(0.0, 10, nullptr, ix.data(), jx.data(), el.data()) == NBODY_ERR_ARG);
    CHECK(nbody_binaries(0.0, 0, nullptr, nullptr, nullptr, nullptr) == NBODY_ERR_ARG);
    CHECK(nbody_binaries(0.0, 10, &found, nullptr, jx.data(), el.data()) == NBODY_ERR_ARG);
    CHECK(nbody_binaries(0.0, 10, &found, ix.data(), nullptr, el.data()) == NBODY_ERR_ARG);
    CHECK(nbody_binaries(0.0, 10, &found, ix.data(), jx.data(), nullptr) == NBODY_ERR_ARG);
    CHECK(nothing_beyond(e, 0) && nothing_beyond(ix, 0) && nothing_beyond(jx, 0) && nothing_beyond(el, 0) && found == kMark);
    std::vector<double> ed(2085, 5.0);
    CHECK(nbody_pair_energy_rows_d(0, 2085, ed.data(), ix.data()) == NBODY_ERR_STATE && ed[0] == 5.0 && ed[2084] == 5.0 && ix[0] == kMark);
    c.run_all();
    CHECK(c.run_binaries(-0.0, 2085) == c.run_binaries(0.0, 2085));   // e_max = -0 is 0
    SHUTDOWN();
    Case<double> d(1000);
    d.open(1);
    CHECK(nbody_pair_energy_rows(0, 1000, e.data(), ix.data()) == NBODY_ERR_STATE);
    d.run_all();   // nbody_binaries serves both precisions
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(2085);
    const int gather = ngpus > 1 ? 1 : 0;   // ts_vel, where the velocities have to travel
    env.set("3", nullptr);
    int made = sweep("nbody_pair_energy_rows split", [&] { c.open(ngpus); }, [&] { return nbody_pair_energy_rows(0, c.n, c.e.data(), c.idx.data()); },
                     [&] { c.run(); });
    CHECK(made == (3 + gather) * ngpus);   // e, idx, scratch per device
    env.set("1", nullptr);
    made = sweep("nbody_pair_energy_rows", [&] { c.open(ngpus); }, [&] { return nbody_pair_energy_rows(0, c.n, c.e.data(), nullptr); },
                 [&] { c.run(0, -1, 1); });
    CHECK(made == (1 + gather) * ngpus);   // e
    int found = 0;
    std::vector<int> gi(2085), gj(2085);
    std::vector<double> el(2085 * NBODY_BINARY_WORDS);
    made = sweep("nbody_binaries", [&] { c.open(ngpus); }, [&] { return nbody_binaries(0.0, 2085, &found, gi.data(), gj.data(), el.data()); },
                 [&] { c.run_binaries(0.0, 2085); });
    CHECK(made == (2 + gather) * ngpus);   // e, idx per device
    env.set("2", nullptr);
    made = sweep("nbody_binaries split", [&] { c.open(ngpus); }, [&] { return nbody_binaries(0.0, 0, &found, nullptr, nullptr, nullptr); },
                 [&] { c.run_binaries(0.0, 0); });
    CHECK(made == (3 + gather) * ngpus);   // e, idx, scratch per device
  });
  env.set(nullptr, nullptr);
  printf("pair_energy_sanity ok\n");
  return 0;
}
