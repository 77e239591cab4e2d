// host_sanity.cpp — TEST INFRASTRUCTURE: drives the C-ABI of include/nbody.h on top of hip_stub.cpp (no GPU) so that the library's HOST
// code runs under sanitizers.  usage: host_sanity [serve_requests [mailbox-only]]   exit code 0 = every check held.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#define SANITY_NAME "host_sanity"
#include "sanity_common.hpp"

extern "C" void hip_stub_lose_next_completion(void);   // hip_stub.cpp

static void bodies(std::vector<float>& p, int n, unsigned seed) {
  p.resize((size_t)n * 4);
  unsigned s = seed * 2654435761u + 12345u;
  for (auto& v : p) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) / 8388608.0f - 1.0f; }
}

static long long info(int key) { long long v = -1; OK(nbody_get_info(key, &v)); return v; }

// nbody_energy and nbody_potential_rows(_d) on the uploaded state, against what the stub's energy pass writes (hip_stub.cpp energy()):
// phi of body i = x_i - i; totals {n / 2, n, sum of vel.x, 4n, 5n, 6n, 7n, 8n}.  Windows: all rows, one across the first two slices of a
// three-device context (N = 1001: 0..333 | 334..667), the last row; and ranges that leave the context's rows.
template <typename T>
static void check_energy(int n, const std::vector<T>& pos, const std::vector<T>& vel, int (*potential_rows)(int, int, T*)) {
  double e[NBODY_ENERGY_WORDS];
  OK(nbody_energy(e));
  double px = 0.0, ax = 0.0;
  for (int i = 0; i < n; ++i) { px += (double)vel[(size_t)i * 4]; ax += fabs((double)vel[(size_t)i * 4]); }
  for (int q = 0; q < NBODY_ENERGY_WORDS; ++q)
    CHECK(q == 2 ? fabs(e[q] - px) <= 1e-9 * (1.0 + ax) : e[q] == (q < 2 ? 0.5 : 1.0) * (q + 1) * (double)n);
  const int mid = n / 3 > 50 ? n / 3 - 50 : 0;
  const int windows[3][2] = {{0, n}, {mid, n - mid < 100 ? n - mid : 100}, {n - 1, 1}};
  for (const auto& w : windows) {
    std::vector<T> phi((size_t)w[1] + 1, (T)-1);
    OK(potential_rows(w[0], w[1], phi.data()));
    for (int k = 0; k < w[1]; ++k) CHECK(phi[k] == pos[(size_t)(w[0] + k) * 4] - (T)(w[0] + k));
    CHECK(phi[w[1]] == (T)-1);
  }
  T buf[4];
  CHECK(potential_rows(n - 1, 2, buf) == NBODY_ERR_ARG && potential_rows(-1, 1, buf) == NBODY_ERR_ARG && potential_rows(0, 0, buf) == NBODY_ERR_ARG);
}

// the bodies of seeds (1, 2) uploaded and stepped `steps` times (or, step_now = false, the context as the caller stepped it):
// positions and velocities back as {pos, vel}
static std::vector<float> stepped(int n, int steps, bool step_now = true) {
  std::vector<float> p, v, out((size_t)n * 8);
  bodies(p, n, 1); bodies(v, n, 2);
  BodySystem b = {p.data(), v.data()};
  if (step_now) { OK(nbody_upload(&b)); OK(nbody_step(0.01f, steps)); }
  OK(nbody_sync());
  BodySystem o = {out.data(), out.data() + (size_t)n * 4};
  OK(nbody_download(&o));
  CHECK(info(NBODY_INFO_STEPS_DONE) == steps);
  return out;
}

// the failure paths of everything that creates a resource: sweep() (sanity_common.hpp) walks every creating call of an entry point,
// the timer rings' 2 x 2 x 256 events per local included
static void failure_sweeps() {
  const int n = 200, n3 = 100;   // n3: ragged over three devices (34, 33, 33)
  std::vector<float> pos, vel;
  bodies(pos, n, 1); bodies(vel, n, 2);
  BodySystem b = {pos.data(), vel.data()};
  auto fresh = [&] { OK(nbody_init(n, 1, 0, 0)); OK(nbody_upload(&b)); };
  // what the calls give on contexts that never saw a failure
  OK(nbody_init(n, 1, 0, 0));
  const std::vector<float> want4 = stepped(n, 4);
  SHUTDOWN();
  fresh();
  const std::vector<float> want70 = stepped(n, 70);
  OK(nbody_set_option(NBODY_OPT_JSUB, 64));
  std::vector<float> wantf((size_t)n * 4), f((size_t)n * 4);
  OK(nbody_forces(pos.data(), wantf.data(), n));
  SHUTDOWN();

  int made = sweep("nbody_init", [] {}, [&] { return nbody_init(n, 1, 0, 0); }, [&] { CHECK(info(NBODY_INFO_N) == n && stepped(n, 4) == want4); });
  CHECK(made >= 2 + 5 + 3 + 4 * 256);   // streams, buffers, events and both timer rings were all walked
  if (three_devices()) {
    OK(nbody_init(n3, 3, 0, 0));
    const std::vector<float> want3 = stepped(n3, 4);
    SHUTDOWN();
    made = sweep("nbody_init x 3", [] {}, [&] { return nbody_init(n3, 3, 0, 0); }, [&] { CHECK(info(NBODY_INFO_NRANKS) == 3 && stepped(n3, 4) == want3); });
    CHECK(made >= 3 * (2 + 5 + 5 + 4 * 256));
  }
  made = sweep("nbody_init_rank", [] {}, [&] { return nbody_init_rank(n3, 0, 0, 1, 3, nullptr); },
               [&] { CHECK(info(NBODY_INFO_NRANKS) == 3 && info(NBODY_INFO_RANK) == 1 && info(NBODY_INFO_FIRST_BODY) == 34 && info(NBODY_INFO_N_LOCAL) == 33); });
  CHECK(made >= 2 + 5 + 5 + 4 * 256);
  {  // the mailbox in its faithful mode (the strict proof allocates too): one request's RAM B against a context that never saw a failure
    std::vector<uint32_t> a((size_t)(64 + 1) * 4), want_b;
    std::vector<float> rb((size_t)(64 + 1) * 4);
    auto request = [&] {
      a[0] = 1; a[1] = 9; a[2] = a[3] = 0; memcpy(a.data() + 4, pos.data(), 9 * 16);
      OK(nbody_mailbox_run(a.data(), rb.data(), 300000));
      return std::vector<uint32_t>((uint32_t*)rb.data() + 4, (uint32_t*)rb.data() + 4 + 9 * 4);
    };
    OK(nbody_mailbox_open(64, 1));
    want_b = request();
    SHUTDOWN();
    made = sweep("nbody_mailbox_open", [] {}, [] { return nbody_mailbox_open(64, 1); }, [&] { CHECK(info(NBODY_INFO_N) == 64 && request() == want_b); });
    CHECK(made >= 2 + 5 + 3 + 4 * 256 + 4);
  }
  double e[NBODY_ENERGY_WORDS];
  std::vector<float> phi(n);
  made = sweep("nbody_energy", fresh, [&] { return nbody_energy(e); }, [&] { check_energy(n, pos, vel, nbody_potential_rows); });
  CHECK(made == 3);
  made = sweep("nbody_potential_rows", fresh, [&] { return nbody_potential_rows(0, n, phi.data()); }, [&] { check_energy(n, pos, vel, nbody_potential_rows); });
  CHECK(made == 3);
  made = sweep("nbody_step", fresh, [] { return nbody_step(0.01f, 70); }, [&] { CHECK(stepped(n, 70, false) == want70); });   // capture and instantiate
  CHECK(made == 1);
  made = sweep("nbody_forces", fresh, [&] { int rc = nbody_set_option(NBODY_OPT_JSUB, 64); return rc ? rc : nbody_forces(pos.data(), f.data(), n); },
               [&] { CHECK(f == wantf); });                                                   // 64 segments: the partial sums grow
  CHECK(made == 1);
}

int main(int argc, char** argv) {
  const int serve_requests = argc > 1 ? atoi(argv[1]) : 10000;
  const bool mailbox_only = argc > 2;
  std::vector<float> pos, vel, p2, v2, f, f2;
  // ---- a context, the step loop with its graphs, forces, row windows, options that re-segment ----
  for (int n : {1, 63, 1000, 2085}) {
    if (mailbox_only) break;
    bodies(pos, n, 1); bodies(vel, n, 2);
    OK(nbody_init(n, 1, 0, 0));
    BodySystem b = {pos.data(), vel.data()};
    OK(nbody_upload(&b));
    check_energy(n, pos, vel, nbody_potential_rows);
    OK(nbody_step(0.01f, 70));                     // one eager step, graphs of 32 + the rest
    OK(nbody_sync());
    p2.assign((size_t)n * 4, 0.f); v2.assign((size_t)n * 4, 0.f);
    BodySystem o = {p2.data(), v2.data()};
    OK(nbody_download(&o));
    CHECK(info(NBODY_INFO_STEPS_DONE) == 70);
    f.assign((size_t)n * 4, 0.f);
    OK(nbody_forces(pos.data(), f.data(), n));
    for (int jsub : {1, 3, 64}) for (int fuse : {0, 1}) for (int ws : {1, 4, 16}) {
      OK(nbody_set_option(NBODY_OPT_JSUB, jsub)); OK(nbody_set_option(NBODY_OPT_FUSE_COMBINE, fuse)); OK(nbody_set_option(NBODY_OPT_WSPLIT, ws));
      f2.assign((size_t)n * 4, -1.f);
      OK(nbody_forces(pos.data(), f2.data(), n));
      if (n > 1) { const int r0 = n / 3, nr = n - r0 < 100 ? n - r0 : 100; std::vector<float> w((size_t)nr * 4); OK(nbody_forces_rows(r0, nr, w.data())); }
      OK(nbody_upload(&b)); OK(nbody_step(0.01f, 5));
    }
    OK(nbody_set_option(NBODY_OPT_SUM_ORDER, NBODY_SUM_FPGA16)); OK(nbody_set_option(NBODY_OPT_JSUB, 1)); OK(nbody_set_option(NBODY_OPT_WSPLIT, -1));
    OK(nbody_forces(pos.data(), f2.data(), n));
    CHECK(bodyForce(pos.data(), vel.data(), 0.01f, n) == 0 && integrate(pos.data(), vel.data(), 0.01f, n) == 0);
    SHUTDOWN();
  }
  if (!mailbox_only) {  // fp64, and one process driving three (stub) devices: peer copies, ragged slices
    const int n = 1001;
    std::vector<double> dp((size_t)n * 4, 0.25), dv((size_t)n * 4, 0.0);
    for (size_t k = 0; k < dp.size(); ++k) dp[k] = (double)((k * 2654435761u) % 1000) / 1000.0;
    OK(nbody_init(n, 1, 1, 0));
    BodySystemD b = {dp.data(), dv.data()};
    OK(nbody_upload_d(&b)); OK(nbody_step_d(0.01, 9)); OK(nbody_download_d(&b));
    check_energy(n, dp, dv, nbody_potential_rows_d);
    CHECK(nbody_step(0.01f, 1) == NBODY_ERR_STATE);
    SHUTDOWN();
    if (three_devices()) {
      bodies(pos, n, 5); bodies(vel, n, 6);
      OK(nbody_init(n, 3, 0, 0));
      BodySystem bb = {pos.data(), vel.data()};
      for (int ov : {0, 1, 2}) { OK(nbody_set_option(NBODY_OPT_OVERLAP, ov)); OK(nbody_upload(&bb)); OK(nbody_step(0.01f, 4)); OK(nbody_download(&bb)); }
      check_energy(n, pos, vel, nbody_potential_rows);                // after steps: the other slices are brought over first
      f.assign((size_t)n * 4, 0.f);
      OK(nbody_forces(pos.data(), f.data(), n));
      SHUTDOWN();
    }
  }
  if (!mailbox_only) failure_sweeps();
  // ---- the mailbox: the address map, every form, the guard ----
  const int cap = 700;
  OK(nbody_mailbox_open(cap, 0));
  uint32_t* ram_a; float* ram_b; int c = 0;
  OK(nbody_mailbox_rams((void**)&ram_a, (void**)&ram_b, &c));
  CHECK(c == cap);
  bodies(pos, cap, 9); bodies(vel, cap, 10);
  {  // the energy entry points on the mailbox's context, before a request overwrites its position buffer
    BodySystem b = {pos.data(), vel.data()};
    OK(nbody_upload(&b));
    check_energy(cap, pos, vel, nbody_potential_rows);
  }
  std::vector<std::vector<uint32_t>> first(cap + 1);
  auto post = [&](int n) { memcpy(ram_a + 4, pos.data(), (size_t)n * 16); ram_a[1] = (uint32_t)n; ram_a[2] = ram_a[3] = 0; };
  auto check_b = [&](const float* rb, int n, int words) {
    const uint32_t* w = (const uint32_t*)rb;
    for (int k = 0; k < 4; ++k) CHECK(w[k] == 0xDEADBEEFu);                                   // word 0 of RAM B is never written
    for (int k = (n + 1) * 4; k < words * 4; ++k) CHECK(w[k] == 0xDEADBEEFu);                  // nor the words beyond N
    std::vector<uint32_t> got(w + 4, w + 4 + (size_t)n * 4);
    if (first[n].empty()) first[n] = got;
    CHECK(got == first[n]);
  };
  auto fill = [&](float* rb, int words) { for (int k = 0; k < words * 4; ++k) ((uint32_t*)rb)[k] = 0xDEADBEEFu; };
  std::vector<uint32_t> own_a((size_t)(cap + 1) * 4);
  std::vector<float> own_b((size_t)(cap + 1) * 4);
  for (int round = 0; round < 3; ++round)
    for (int n : {9, 700, 0, 1, 64, 65, 300, 2, 3}) {
      fill(ram_b, cap + 1); post(n); ram_a[0] = 1;
      OK(nbody_mailbox_run(ram_a, ram_b, 300000));
      CHECK((ram_a[0] & 1u) == 0 && ram_a[1] >= 1 && ram_a[2] == 0 && ram_a[3] == 0);
      check_b(ram_b, n, cap + 1);
      fill(own_b.data(), cap + 1);
      own_a[0] = 1; own_a[1] = (uint32_t)n; own_a[2] = own_a[3] = 0; memcpy(own_a.data() + 4, pos.data(), (size_t)n * 16);
      OK(nbody_mailbox_run(own_a.data(), own_b.data(), 300000));                               // the caller's own images
      CHECK((own_a[0] & 1u) == 0 && own_a[1] >= 1);
      check_b(own_b.data(), n, cap + 1);
      CHECK(info(NBODY_INFO_N) == cap);
    }
  ram_a[0] = 0; CHECK(nbody_mailbox_run(ram_a, ram_b, 0) == NBODY_ERR_STATE);
  ram_a[0] = 1; ram_a[1] = cap + 1; CHECK(nbody_mailbox_run(ram_a, ram_b, 0) == NBODY_ERR_ARG);
  ram_a[0] = 0;                                                                                // (a refused call leaves BEGIN as the caller set it: nothing may be pending when the thread starts)
  // served: this thread posts and polls, a second thread hammers nbody_get_info and the refused entry points
  const long long n0 = info(NBODY_INFO_N), nseg0 = info(NBODY_INFO_NSEG), sub0 = info(NBODY_INFO_JSUB), ws0 = info(NBODY_INFO_WSPLIT);
  OK(nbody_mailbox_serve(1, 300000));
  std::atomic<int> stop{0}, bad{0};
  std::atomic<long long> looked{0};
  std::thread hammer([&] {
    std::vector<float> buf((size_t)cap * 4);
    BodySystem bs = {buf.data(), buf.data()};
    int k = 0;
    while (!stop.load(std::memory_order_acquire)) {
      long long v;
      if (nbody_get_info(NBODY_INFO_N, &v) || v != n0) bad++;
      if (nbody_get_info(NBODY_INFO_NSEG, &v) || v != nseg0) bad++;
      if (nbody_get_info(NBODY_INFO_JSUB, &v) || v != sub0) bad++;
      if (nbody_get_info(NBODY_INFO_WSPLIT, &v) || v != ws0) bad++;
      if (nbody_get_info(NBODY_INFO_MAILBOX_SERVING, &v) || v != 1) bad++;
      int rc;
      double e[NBODY_ENERGY_WORDS];
      switch (k++ % 11) {
        case 0: rc = nbody_step(0.01f, 1); break;
        case 1: rc = nbody_set_option(NBODY_OPT_JSUB, 2); break;
        case 2: rc = nbody_upload(&bs); break;
        case 3: rc = nbody_download(&bs); break;
        case 4: rc = nbody_forces(buf.data(), buf.data(), cap); break;
        case 5: rc = nbody_sync(); break;
        case 6: rc = nbody_mailbox_open(64, 0); break;
        case 7: rc = nbody_init(64, 1, 0, 0); break;
        case 8: rc = nbody_energy(e); break;
        case 9: rc = nbody_potential_rows(0, 1, buf.data()); break;
        default: rc = nbody_mailbox_run(ram_a, ram_b, 0); break;
      }
      if (rc != NBODY_ERR_STATE) bad++;
      looked++;
    }
  });
  const int sizes[] = {9, 700, 40, 1, 333, 0, 64};
  for (int k = 0; k < serve_requests; ++k) {
    const int n = sizes[k % 7];
    if (k % 97 == 0) fill(ram_b, cap + 1);
    post(n);
    __atomic_store_n(&ram_a[0], 1u, __ATOMIC_RELEASE);
    while (__atomic_load_n(&ram_a[0], __ATOMIC_ACQUIRE) & 1u) { }
    CHECK(ram_a[3] == 0 && ram_a[1] >= 1);
    if (k % 97 == 0) check_b(ram_b, n, cap + 1);
    else { std::vector<uint32_t> got((uint32_t*)ram_b + 4, (uint32_t*)ram_b + 4 + (size_t)n * 4); CHECK(first[n].empty() || got == first[n]); }
  }
  stop.store(1, std::memory_order_release);
  hammer.join();
  CHECK(bad.load() == 0 && looked.load() > 0);
  long long served = 0;
  for (int spin = 0; spin < 1000000 && served < serve_requests; ++spin) served = info(NBODY_INFO_MAILBOX_SERVED);
  CHECK(served == serve_requests);
  OK(nbody_mailbox_serve(0, 0));
  OK(nbody_sync());                                                                            // the context is the caller's again
  fill(ram_b, cap + 1); post(300); ram_a[0] = 1;
  OK(nbody_mailbox_run(ram_a, ram_b, 0));
  check_b(ram_b, 300, cap + 1);
  // a request whose completion wait fails (the stub loses the completion and leaves an arrival counter part-counted): the next request
  // must start from clean counters.  Several segments combined by the last arriver, so that the counters are in use.
  OK(nbody_set_option(NBODY_OPT_FUSE_COMBINE, 1)); OK(nbody_set_option(NBODY_OPT_JSUB, 3));
  std::vector<uint32_t> want;
  for (int k = 0; k < 3; ++k) {
    fill(ram_b, cap + 1); post(300); ram_a[0] = 1;
    if (k == 1) { hip_stub_lose_next_completion(); CHECK(nbody_mailbox_run(ram_a, ram_b, 0) == NBODY_ERR_STATE); continue; }
    OK(nbody_mailbox_run(ram_a, ram_b, 0));
    std::vector<uint32_t> got((uint32_t*)ram_b + 4, (uint32_t*)ram_b + 4 + 300 * 4);
    for (uint32_t v : got) CHECK(v != 0xDEADBEEFu);
    if (k == 0) want = got;
    else CHECK(got == want);
  }
  OK(nbody_mailbox_serve(1, 0));                                                               // shutdown with the thread still serving
  SHUTDOWN();
  printf("host_sanity ok: %d served requests, %lld looks by the second thread\n", serve_requests, looked.load());
  return 0;
}
