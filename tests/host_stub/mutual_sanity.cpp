// mutual_sanity.cpp — TEST INFRASTRUCTURE (tests/test_mutual_host_sanitizers.py): drives NBODY_OPT_PAIRING through the library's host code
// (context.cpp, comm.cpp, mailbox.cpp, energy.cpp, mutual.cpp) against mutual_stub.cpp under AddressSanitizer + UBSan.  What it checks is
// the host's logic: which passes take the mutual pairing and which are refused, the table and the counters (the stand-in aborts unless
// every word of the table is written exactly once and every counter returns to zero), the step loop with its captured graphs, the
// option's values and read-back, a table that cannot be allocated (the pass runs ordered and says so, until the option is set again),
// and that nbody_shutdown leaves nothing.
#include <math.h>
#include <string.h>

#define SANITY_NAME "mutual_sanity"
#include "sanity_common.hpp"

extern "C" long mutual_stub_launches(void);

static long long info(int key) { long long v = -1; OK(nbody_get_info(key, &v)); return v; }

static void bodies(std::vector<float>& p, int n, unsigned seed) {
  p.resize((size_t)n * 4);
  unsigned s = seed * 2654435761u + 12345u;
  for (auto& v : p) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) / 8388608.0f - 1.0f; }
}

// the stand-in's two forms add the same terms in different orders
static bool close_to(const std::vector<float>& a, const std::vector<float>& b) {
  for (size_t k = 0; k < a.size(); ++k) if (fabsf(a[k] - b[k]) > 1e-3f * (1.f + fabsf(b[k]))) return false;
  return true;
}

static std::vector<float> state(int n) {   // positions and velocities as the context holds them
  std::vector<float> out((size_t)n * 8);
  BodySystem o = {out.data(), out.data() + (size_t)n * 4};
  OK(nbody_sync()); OK(nbody_download(&o));
  return out;
}

int main() {
  std::vector<float> pos, vel, f, f2;
  for (int nb : {1, 2, 3, 4}) {
    const int n = 1024 * nb;
    const long base = mutual_stub_launches();   // the stand-in counts over the whole program
    bodies(pos, n, 21); bodies(vel, n, 22);
    OK(nbody_init(n, 1, 0, 0));
    BodySystem b = {pos.data(), vel.data()};
    OK(nbody_set_option(NBODY_OPT_JSUB, nb % 3 == 0 ? 3 : 1)); OK(nbody_set_option(NBODY_OPT_WSPLIT, 1));
    CHECK(info(NBODY_INFO_PAIRING) == NBODY_PAIRING_ORDERED);                  // AUTO below 2^20 rows
    f.assign((size_t)n * 4, 0.f); f2.assign((size_t)n * 4, -1.f);
    OK(nbody_forces(pos.data(), f.data(), n));
    OK(nbody_upload(&b)); OK(nbody_step(0.01f, 5));
    const std::vector<float> want = state(n);
    CHECK(mutual_stub_launches() == base);
    OK(nbody_set_option(NBODY_OPT_PAIRING, NBODY_PAIRING_MUTUAL));
    CHECK(info(NBODY_INFO_PAIRING) == NBODY_PAIRING_MUTUAL && info(NBODY_INFO_LAUNCHES_PER_STEP) == 1);
    OK(nbody_forces(pos.data(), f2.data(), n));
    CHECK(close_to(f2, f) && mutual_stub_launches() == base + 1);
    OK(nbody_forces_rows(0, n, f2.data()));                                     // all rows: a full pass
    CHECK(nbody_forces_rows(1, n - 1, f2.data()) == NBODY_ERR_UNSUPPORTED);     // a window is not
    OK(nbody_upload(&b)); OK(nbody_step(0.01f, 5));                             // one eager step, then captured graphs
    CHECK(close_to(state(n), want) && mutual_stub_launches() == base + 2 + 5);
    OK(nbody_set_option(NBODY_OPT_SUM_BLOCK, 512));
    CHECK(nbody_step(0.01f, 1) == NBODY_ERR_UNSUPPORTED && nbody_forces(pos.data(), f2.data(), n) == NBODY_ERR_UNSUPPORTED);
    OK(nbody_set_option(NBODY_OPT_SUM_BLOCK, 1024));
    if (nb > 1) {   // pieces that are not whole blocks
      OK(nbody_set_option(NBODY_OPT_WSPLIT, 16)); OK(nbody_set_option(NBODY_OPT_JSUB, 5));
      CHECK(nbody_forces(pos.data(), f2.data(), n) == NBODY_ERR_UNSUPPORTED && info(NBODY_INFO_PAIRING) == NBODY_PAIRING_ORDERED);
      OK(nbody_set_option(NBODY_OPT_JSUB, nb % 3 == 0 ? 3 : 1)); OK(nbody_set_option(NBODY_OPT_WSPLIT, 1));
    }
    // the table cannot be allocated (the counters' allocation fails, then the table's): the pass runs ordered and says so
    for (int k : {1, 2}) {
      OK(nbody_set_option(NBODY_OPT_PAIRING, NBODY_PAIRING_MUTUAL));
      const long launches = mutual_stub_launches();
      hip_stub_fail_nth(k);
      OK(nbody_forces(pos.data(), f2.data(), n));
      CHECK(hip_stub_fail_pending() == 0 && f2 == f && mutual_stub_launches() == launches && info(NBODY_INFO_PAIRING) == NBODY_PAIRING_NO_TABLE);
      OK(nbody_step(0.01f, 5));
      CHECK(mutual_stub_launches() == launches);
    }
    OK(nbody_set_option(NBODY_OPT_PAIRING, NBODY_PAIRING_MUTUAL));             // set again: tried again
    OK(nbody_forces(pos.data(), f2.data(), n));
    CHECK(info(NBODY_INFO_PAIRING) == NBODY_PAIRING_MUTUAL && close_to(f2, f));
    OK(nbody_set_option(NBODY_OPT_PAIRING, NBODY_PAIRING_AUTO));
    CHECK(info(NBODY_INFO_PAIRING) == NBODY_PAIRING_ORDERED);
    CHECK(nbody_set_option(NBODY_OPT_PAIRING, 3) == NBODY_ERR_ARG && nbody_set_option(NBODY_OPT_PAIRING, -1) == NBODY_ERR_ARG);
    SHUTDOWN();
  }
  {  // not a multiple of 1024, fp64, three devices: MUTUAL is refused, AUTO is ORDERED
    bodies(pos, 1500, 23);
    OK(nbody_init(1500, 1, 0, 0));
    OK(nbody_set_option(NBODY_OPT_PAIRING, NBODY_PAIRING_MUTUAL));
    f.assign((size_t)1500 * 4, 0.f);
    CHECK(nbody_forces(pos.data(), f.data(), 1500) == NBODY_ERR_UNSUPPORTED && nbody_step(0.01f, 1) == NBODY_ERR_UNSUPPORTED);
    SHUTDOWN();
    OK(nbody_init(2048, 1, 1, 0));
    OK(nbody_set_option(NBODY_OPT_PAIRING, NBODY_PAIRING_MUTUAL));
    CHECK(nbody_step_d(0.01, 1) == NBODY_ERR_UNSUPPORTED && info(NBODY_INFO_PAIRING) == NBODY_PAIRING_ORDERED);
    SHUTDOWN();
    if (three_devices()) {
      OK(nbody_init(3072, 3, 0, 0));
      OK(nbody_set_option(NBODY_OPT_PAIRING, NBODY_PAIRING_MUTUAL));
      CHECK(nbody_step(0.01f, 1) == NBODY_ERR_UNSUPPORTED);
      SHUTDOWN();
    }
  }
  printf("mutual_sanity ok\n");
  return 0;
}
