// hermite6_block_sanity.cpp — TEST INFRASTRUCTURE (tests/test_hermite6_block_host_sanitizers.py): drives nbody_step_hermite6_block(_d) of
// the library's host code (hermite6_block.cpp on hermite6.cpp's opening, hermite_block.cpp's next-time read, hermite.cpp's gathers and
// point_sums.cpp beside context.cpp, comm.cpp, mailbox.cpp, energy.cpp) against tests/host_stub/hip_stub.cpp, snap_stub.cpp,
// hermite_stub.cpp, hermite_block_stub.cpp, hermite6_stub.cpp and hermite6_block_stub.cpp under AddressSanitizer + UBSan.
// What it checks is the host's logic: the buffers of a call on every device, the fold of the devices' next-time words, the predicted
// positions, velocities AND accelerations of ALL bodies reaching every device in every sub-step (snap_stub.cpp's values of a row depend
// on the first source of every block and on the last body in all three streams: a device that evaluated on a stale slice is found
// out), the snap points pass over queries left on the device — its split and batches — with the three outputs indexed by the active
// list, a device WITHOUT an active row, the counters, the argument checks, lifetimes at shutdown and the failure paths.  The
// expectations come from a model of the stubs, operation for operation, over the whole system.  It covers N = 1, 1000 and 2085 on one
// stub device and three with ragged slices, one level (against nbody_step_hermite6 itself) and eight, one and two blocks, the source
// split forced (3 chunks; 2 in the interleaved calls, 1 in the sweep) and automatic, the batched path under a small scratch bound,
// block calls interleaved with nbody_step_hermite6, nbody_step_hermite_block and nbody_snap_rows on one context, every NBODY_ERR_ARG
// case and the failure sweep of sanity_common.hpp.
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>

#include <limits>

#define SANITY_NAME "hermite6_block_sanity"
#include "sanity_common.hpp"

static const SplitEnv env = {"NBODY_SNAP_SPLIT", "NBODY_SNAP_SCRATCH_MB"};

static int block6(float, double eta, double dt, int levels, int nb, long long* s, long long* e) { return nbody_step_hermite6_block((float)eta, (float)dt, levels, nb, s, e); }
static int block6(double, double eta, double dt, int levels, int nb, long long* s, long long* e) { return nbody_step_hermite6_block_d(eta, dt, levels, nb, s, e); }
static int block4(float, double eta, double dt, int levels, int nb) { return nbody_step_hermite_block((float)eta, (float)dt, levels, nb, nullptr, nullptr); }
static int block4(double, double eta, double dt, int levels, int nb) { return nbody_step_hermite_block_d(eta, dt, levels, nb, nullptr, nullptr); }
static int hermite6(float, double dt, int k) { return nbody_step_hermite6((float)dt, k); }
static int hermite6(double, double dt, int k) { return nbody_step_hermite6_d(dt, k); }
static int snap_rows(int f, int m, float* a, float* j, float* s) { return nbody_snap_rows(f, m, a, j, s); }
static int snap_rows(int f, int m, double* a, double* j, double* s) { return nbody_snap_rows_d(f, m, a, j, s); }
template <typename T> int download(std::vector<T>& pos, std::vector<T>& vel);
template <> int download<float>(std::vector<float>& pos, std::vector<float>& vel) { BodySystem b = {pos.data(), vel.data()}; return nbody_download(&b); }
template <> int download<double>(std::vector<double>& pos, std::vector<double>& vel) { BodySystemD b = {pos.data(), vel.data()}; return nbody_download_d(&b); }

// the model: the scheme of include/nbody.h over the whole system, with snap_stub.cpp's (a, j, s) of a row at a state of all bodies
template <typename T>
struct Model {
  int n, nb, levels;
  T unit;
  double eta2, lim[24];
  std::vector<T> pos, vel, ap, x0, v0, a0, j0, s0, c0;
  std::vector<long long> t0;
  std::vector<int> lev;
  long long steps = 0, evals = 0;
  int idle_substeps = 0, one_row_substeps = 0, seen_levels = 0;

  // snap_stub.cpp's nine values of row i — query (p_i, v_i, g_i), skip = i — at the state (p, v, g) of all bodies; s may be null
  void eval_row(const std::vector<T>& p, const std::vector<T>& v, const std::vector<T>& g, int i, T* a, T* j, T* s) const {
    const T* me = &p[4 * (size_t)i];
    const T* mv = &v[4 * (size_t)i];
    const T* ma = &g[4 * (size_t)i];
    double q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nb; ++b) {
      const size_t b0 = 4 * (size_t)b * stub::kBlock, jn = 4 * (size_t)(n - 1);
      const bool last = b == nb - 1;
      q[0] += (double)(T)(p[b0] - me[0]);
      q[1] += (double)(T)(v[b0] - mv[0]);
      q[2] += (double)(T)((T)i + (last ? p[jn] : (T)0));
      q[3] += (double)(T)(mv[1] + (last ? v[jn] : (T)0));
      q[4] += (double)me[3];
      q[5] += (double)mv[3];
      q[6] += (double)(T)(g[b0] - ma[0]);
      q[7] += (double)(T)(ma[1] + (last ? g[jn] : (T)0));
      q[8] += (double)ma[3];
    }
    for (int c = 0; c < 3; ++c) { a[c] = (T)q[c]; j[c] = (T)q[3 + c]; if (s) s[c] = (T)q[6 + c]; }
    a[3] = (T)0; j[3] = (T)0;
    if (s) s[3] = (T)0;
  }
  int want(const T* a, const T* j) const {
    const double ax = (double)a[0], ay = (double)a[1], az = (double)a[2], jx = (double)j[0], jy = (double)j[1], jz = (double)j[2];
    const double a2 = (ax * ax + ay * ay) + az * az, j2 = (jx * jx + jy * jy) + jz * jz;
    const double q = a2 / j2;
    if (!(q < std::numeric_limits<double>::infinity())) return 0;
    const double e = eta2 * q;
    for (int k = 0; k < levels; ++k)
      if (lim[k] <= e) return k;
    return levels - 1;
  }
  // eta, dt_max: as the entry point of T receives them.  The opening is nbody_snap_rows': the accelerations of the jerk rows pass (the
  // first three values, which do not depend on the accelerations brought), then the nine with them
  Model(const std::vector<T>& p, const std::vector<T>& v, double eta, double dt_max, int levels_)
      : n((int)(p.size() / 4)), nb(stub::blocks_of(n)), levels(levels_), pos(p), vel(v), ap(p.size(), (T)0), x0(p), v0(v), a0(p.size()), j0(p.size()),
        s0(p.size()), c0(p.size(), (T)0), t0((size_t)n, 0), lev((size_t)n) {
    eta = (double)(T)eta; dt_max = (double)(T)dt_max;
    unit = (T)ldexp(dt_max, -(levels - 1));
    eta2 = eta * eta;
    for (int k = 0; k < levels; ++k) { const double dk = ldexp(dt_max, -k); lim[k] = dk * dk; }
    std::vector<T> open(p.size()), scratch(4);
    for (int i = 0; i < n; ++i) eval_row(pos, vel, ap, i, &open[4 * (size_t)i], scratch.data(), nullptr);
    for (int i = 0; i < n; ++i) {
      eval_row(pos, vel, open, i, &a0[4 * (size_t)i], &j0[4 * (size_t)i], &s0[4 * (size_t)i]);
      lev[(size_t)i] = want(&a0[4 * (size_t)i], &j0[4 * (size_t)i]);
      seen_levels |= 1 << lev[(size_t)i];
    }
  }
  // slices: the devices' (first, count), to count the sub-steps in which one of them has no active row
  void run(int nblocks, const std::vector<Window>& slices) {
    const long long end = (long long)nblocks << (levels - 1);
    long long tau = 0;
    std::vector<int> act;
    std::vector<T> a1, j1, s1;
    while (tau < end) {
      tau = std::numeric_limits<long long>::max();
      for (int i = 0; i < n; ++i) tau = std::min(tau, t0[(size_t)i] + (1LL << (levels - 1 - lev[(size_t)i])));
      CHECK(tau <= end);
      act.clear();
      for (int i = 0; i < n; ++i) {
        const long long s = 1LL << (levels - 1 - lev[(size_t)i]);
        CHECK(t0[(size_t)i] % s == 0);   // the invariant
        if (t0[(size_t)i] + s == tau) act.push_back(i);
        const T h = (T)(tau - t0[(size_t)i]) * unit;
        const T h2 = h * h, c2 = h2 * (T)0.5, h3 = h2 * h, c3 = h3 / (T)6, h4 = h2 * h2, c4 = h4 / (T)24, h5 = h4 * h, c5 = h5 / (T)120;
        for (int c = 0; c < 3; ++c) {
          const size_t e = 4 * (size_t)i + c;
          pos[e] = std::fma(c5, c0[e], std::fma(c4, s0[e], std::fma(c3, j0[e], std::fma(c2, a0[e], std::fma(h, v0[e], x0[e])))));
          vel[e] = std::fma(c4, c0[e], std::fma(c3, s0[e], std::fma(c2, j0[e], std::fma(h, a0[e], v0[e]))));
          ap[e] = std::fma(c3, c0[e], std::fma(c2, s0[e], std::fma(h, j0[e], a0[e])));
        }
      }
      if (tau % (1LL << (levels - 1)) == 0) CHECK((int)act.size() == n);
      a1.resize(4 * act.size()); j1.resize(4 * act.size()); s1.resize(4 * act.size());
      for (size_t q = 0; q < act.size(); ++q) eval_row(pos, vel, ap, act[q], &a1[4 * q], &j1[4 * q], &s1[4 * q]);
      bool idle = false;
      for (const Window& w : slices) {
        bool any = false;
        for (int i : act) any = any || (i >= w.first && i < w.first + w.count);
        idle = idle || (w.count > 0 && !any);
      }
      idle_substeps += idle;
      one_row_substeps += act.size() == 1;
      for (size_t q = 0; q < act.size(); ++q) {
        const int i = act[q];
        const T h = (T)(tau - t0[(size_t)i]) * unit;
        const T h2 = h * h, h3 = h2 * h, hh = h * (T)0.5, c10 = h2 / (T)10, c120 = h3 / (T)120, r = (T)1 / h;
        for (int c = 0; c < 3; ++c) {
          const size_t e = 4 * (size_t)i + c, f = 4 * q + c;
          const T ss = s0[e] + s1[f], dj = j0[e] - j1[f], sa = a0[e] + a1[f], sj = j0[e] + j1[f], da = a0[e] - a1[f];
          const T w1 = std::fma(c120, ss, std::fma(c10, dj, std::fma(hh, sa, v0[e])));
          const T sv = v0[e] + w1;
          const T y1 = std::fma(c120, sj, std::fma(c10, da, std::fma(hh, sv, x0[e])));
          const T d1 = a1[f] - a0[e];
          const T e1 = (T)60 * d1, p24 = (T)24 * j0[e], m3 = (T)-3 * s0[e];
          const T e2 = std::fma((T)36, j1[f], p24), e3 = std::fma((T)9, s1[f], m3);
          const T in = std::fma(r, std::fma(r, e1, -e2), e3);
          v0[e] = w1; x0[e] = y1; a0[e] = a1[f]; j0[e] = j1[f]; s0[e] = s1[f]; c0[e] = r * in;
          pos[e] = y1; vel[e] = w1;
        }
        t0[(size_t)i] = tau;
        const int w = want(&a1[4 * q], &j1[4 * q]);
        int& k = lev[(size_t)i];
        if (w > k) k = w;
        else if (w < k && tau % (1LL << (levels - k)) == 0) k -= 1;
        seen_levels |= 1 << k;
      }
      ++steps;
      evals += (long long)act.size();
    }
    for (int i = 0; i < n; ++i) CHECK(t0[(size_t)i] == end);
  }
};

static int bits_set(int v) { int c = 0; for (; v; v &= v - 1) ++c; return c; }

// the shared fixture's bodies with velocities: small integers, the w words tag the rows (snap_stub.cpp reads them)
template <typename T>
struct Case : Fixture<T> {
  using Fixture<T>::n; using Fixture<T>::pos; using Fixture<T>::vel;
  std::vector<T> gp, gv, out[3];
  std::vector<Window> slices;
  explicit Case(int n_) : Fixture<T>(n_, 1), gp((size_t)n_ * 4), gv((size_t)n_ * 4) {
    for (auto& o : out) o.resize((size_t)n_ * 4);
    for (int j = 0; j < n; ++j) this->set(vel, j, (T)((j * 7) % 11), (T)(j % 5), (T)2, (T)(j % 31));
  }
  void open_on(int ngpus) {
    this->open(ngpus);
    slices.clear();
    for (int l = 0; l < ngpus; ++l) {
      const int base = n / ngpus, rem = n % ngpus;   // the library's slices: the first n mod ngpus get one row more
      const int f = l * base + std::min(l, rem), e = (l + 1) * base + std::min(l + 1, rem);
      slices.push_back({f, e - f});
    }
  }
  void reset() { OK(upload<T>(pos, vel)); }
  void fetch() { OK(download<T>(gp, gv)); }
  void same_state(const std::vector<T>& p, const std::vector<T>& v) {
    fetch();
    CHECK(!memcmp(gp.data(), p.data(), gp.size() * sizeof(T)) && !memcmp(gv.data(), v.data(), gv.size() * sizeof(T)));
  }
  // a fresh upload and one call against the model: the state bit for bit, the fourth values carried, both counters; NULL counters too
  Model<T> run(double eta, double dt_max, int levels, int nblocks) {
    reset();
    Model<T> m(pos, vel, eta, dt_max, levels);
    m.run(nblocks, slices);
    long long s = -1, e = -1;
    OK(block6(T(), eta, dt_max, levels, nblocks, &s, &e));
    CHECK(s == m.steps && e == m.evals);
    same_state(m.x0, m.v0);
    for (int i = 0; i < n; ++i) CHECK(gp[4 * (size_t)i + 3] == pos[4 * (size_t)i + 3] && gv[4 * (size_t)i + 3] == vel[4 * (size_t)i + 3]);
    reset();
    OK(block6(T(), eta, dt_max, levels, nblocks, nullptr, &e));
    OK(block6(T(), eta, dt_max, levels, 1, &s, nullptr));
    return m;
  }
  // one level is the shared sixth-order step itself, on the same context
  void run_one_level(double dt, int nblocks) {
    reset();
    OK(hermite6(T(), dt, nblocks));
    fetch();
    const std::vector<T> wp = gp, wv = gv;
    reset();
    long long s = -1, e = -1;
    OK(block6(T(), 0.02, dt, 1, nblocks, &s, &e));
    CHECK(s == nblocks && e == (long long)nblocks * n);
    same_state(wp, wv);
  }
  // block calls between calls of the other integrators and nbody_snap_rows on one context: every one sees the state the last one left
  // and finds the shared buffers (he_*, h6_*, hb_*, q_*) fit for its own use
  void run_interleaved() {
    reset();
    OK(hermite6(T(), 0.0078125, 1));
    OK(block4(T(), 0.001953125, 0.0625, 6, 1));
    fetch();
    Model<T> m(gp, gv, 0.001953125, 0.0625, 6);
    m.run(1, slices);
    OK(block6(T(), 0.001953125, 0.0625, 6, 1, nullptr, nullptr));
    same_state(m.x0, m.v0);
    OK(snap_rows(0, n, out[0].data(), out[1].data(), out[2].data()));   // the corrected state of ALL bodies, on every device
    Model<T> after(m.x0, m.v0, 0.001953125, 0.0625, 1);
    for (int o = 0; o < 3; ++o) {
      const std::vector<T>& w = o == 0 ? after.a0 : o == 1 ? after.j0 : after.s0;
      CHECK(!memcmp(out[o].data(), w.data(), w.size() * sizeof(T)));
    }
    OK(block4(T(), 0.001953125, 0.0625, 6, 1));
    OK(hermite6(T(), 0.0078125, 2));
    OK(block6(T(), 0.001953125, 0.0625, 6, 1, nullptr, nullptr));
  }
  void run_all() {
    run_one_level(0.0078125, 1);
    run_one_level(0.01, 3);
    const Model<T> m = run(0.001953125, 0.0625, 8, 1);
    run(0.001953125, 0.0625, 8, 2);
    run(0.5, 0.0625, 3, 1);
    if (n >= 1000) {
      CHECK(bits_set(m.seen_levels) >= 3 && m.evals < m.steps * n);
      if (slices.size() > 1 && n == 2085) CHECK(m.idle_substeps > 0);   // a device with no active row
    }
  }
};

template <typename T>
static void shapes(int n, int ngpus) {
  Case<T> c(n);
  c.open_on(ngpus);
  for_splits(env, {nullptr, "3"}, [&] { c.run_all(); });
  c.run_interleaved();
  env.set("2", nullptr);
  c.run_interleaved();
  env.set(nullptr, nullptr);
  SHUTDOWN();
}

int main() {
  {
    long long s = 5, e = 5;
    CHECK(nbody_step_hermite6_block(0.02f, 0.0625f, 8, 1, &s, &e) == NBODY_ERR_NOT_INIT);
    CHECK(nbody_step_hermite6_block_d(0.02, 0.0625, 8, 1, &s, &e) == NBODY_ERR_NOT_INIT);
    CHECK(s == 5 && e == 5);
  }

  // ---- one block, three blocks with a short last one; one device and three with ragged slices (2085 = 695 x 3, 1000 = 333 + 333 + 334) ----
  for_sizes({1, 1000, 2085}, shapes<float>, shapes<double>);

  // ---- the batched path: 69 blocks of per-block sums per query against 1 MB, fp32: 69 x 36 B = 2484 B, batches of 256 queries ----
  for_device_counts([](int ngpus) {
    Case<float> c(70000);
    c.open_on(ngpus);
    for (const char* split : {(const char*)nullptr, "7"}) {
      env.set(split, "1");
      c.run(0.001953125, 0.0625, 3, 1);
    }
    SHUTDOWN();
  });
  env.set(nullptr, nullptr);

  // ---- the argument checks: nothing is written, the context stays usable ----
  {
    Case<float> c(2085);
    c.open_on(three_devices() ? 3 : 1);
    long long s = 5, e = 5;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    auto bl = [&](float eta, float dt, int levels, int nb) { return nbody_step_hermite6_block(eta, dt, levels, nb, &s, &e); };
    CHECK(bl(0.f, 0.0625f, 8, 1) == NBODY_ERR_ARG && bl(-1.f, 0.0625f, 8, 1) == NBODY_ERR_ARG && bl(nan, 0.0625f, 8, 1) == NBODY_ERR_ARG && bl(inf, 0.0625f, 8, 1) == NBODY_ERR_ARG);
    CHECK(bl(0.02f, 0.f, 8, 1) == NBODY_ERR_ARG && bl(0.02f, -0.0625f, 8, 1) == NBODY_ERR_ARG && bl(0.02f, nan, 8, 1) == NBODY_ERR_ARG && bl(0.02f, inf, 8, 1) == NBODY_ERR_ARG);
    CHECK(bl(0.02f, 0.0625f, 0, 1) == NBODY_ERR_ARG && bl(0.02f, 0.0625f, -1, 1) == NBODY_ERR_ARG && bl(0.02f, 0.0625f, 25, 1) == NBODY_ERR_ARG);
    CHECK(bl(0.02f, 0.0625f, 8, 0) == NBODY_ERR_ARG && bl(0.02f, 0.0625f, 8, -2) == NBODY_ERR_ARG);
    CHECK(bl(0.02f, 1e-37f, 8, 1) == NBODY_ERR_ARG);   // the tick below the smallest normal
    CHECK(nbody_step_hermite6_block_d(0.02, 0.0625, 8, 1, &s, &e) == NBODY_ERR_STATE);
    CHECK(s == 5 && e == 5);
    long long done = -1;
    OK(nbody_get_info(NBODY_INFO_STEPS_DONE, &done));
    CHECK(done == 0);
    c.fetch();
    CHECK(c.gp == c.pos && c.gv == c.vel);   // a refused call has changed nothing in the state
    const Model<float> m = c.run(0.001953125, 0.0625, 8, 1);
    OK(nbody_get_info(NBODY_INFO_STEPS_DONE, &done));
    CHECK(done == 3 * m.steps);   // (run() makes the call three times)
    SHUTDOWN();
    Case<double> d(1000);
    d.open_on(1);
    CHECK(nbody_step_hermite6_block(0.02f, 0.0625f, 8, 1, &s, &e) == NBODY_ERR_STATE);
    CHECK(nbody_step_hermite6_block_d(0.02, 1e-307, 8, 1, &s, &e) == NBODY_ERR_ARG);
    d.run_all();
    SHUTDOWN();
  }

  // ---- the failure paths: every allocating call of a block call, one device and three, split (scratch) and not ----
  for_device_counts([](int ngpus) {
    Case<float> c(2085);
    auto call = [&] { return nbody_step_hermite6_block(0.001953125f, 0.0625f, 5, 1, nullptr, nullptr); };
    auto verify = [&] {
      Model<float> m(c.pos, c.vel, 0.001953125, 0.0625, 5);
      m.run(1, c.slices);
      c.same_state(m.x0, m.v0);
    };
    env.set("3", nullptr);
    const int split = sweep("nbody_step_hermite6_block split", [&] { c.open_on(ngpus); }, call, verify);
    env.set("1", nullptr);
    const int plain = sweep("nbody_step_hermite6_block", [&] { c.open_on(ngpus); }, call, verify);
    const int shared = sweep("nbody_step_hermite6", [&] { c.open_on(ngpus); }, [&] { return nbody_step_hermite6(0.0078125f, 1); }, [&] {});
    // the split call's scratch is one buffer per device more; on top of a shared sixth-order call's: the ranks' next times, ticks,
    // levels, counts, list and the four query buffers, nine per device
    CHECK(split == plain + ngpus && plain == shared + 9 * ngpus);
  });
  env.set(nullptr, nullptr);
  printf("hermite6_block_sanity ok\n");
  return 0;
}
