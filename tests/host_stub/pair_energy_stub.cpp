// pair_energy_stub.cpp — TEST INFRASTRUCTURE (tests/test_pair_energy_host.py): a host-only stand-in for the launch functions of
// pair_energy.hip, linked beside hip_stub.cpp so that pair_energy.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.
// hip_stub.cpp's streams are synchronous and the pass is never captured, so both functions execute at launch.
// The stand-in pushes values a test can predict through the REAL PairEnergyArgs — chunk bounds, the chunks' scratch layout, the combine's
// ascending strict <, pointers the host offset per local and per batch, the rows' first, and BOTH source streams — so ASan sees every
// offset the host computed and a driver sees whether all N velocities arrived.  Per row p (i = first + p, me = src[i], mv = vsrc[i])
// every block b offers the ONE candidate j_b of stub_rule.hpp (steered by me.w; none if j_b == i), of which the stub takes
//   e_b = |src[j_b].x - me.x| - |vsrc[j_b].x - mv.x| - 3
// in ascending b with strict <: symmetric in (i, j_b) as the real e is, of either sign.  It says nothing about the kernels' arithmetic
// (the GPU tests do).
#include <hip/hip_runtime.h>

#include <limits>

#include "../../mini_nbody_amd/csrc/pair_energy_args.hpp"
#include "stub_common.hpp"

namespace {

using namespace nbpe;

template <typename T>
struct Bound { T e; int idx; };

template <typename T>
Bound<T> none() { return {std::numeric_limits<T>::infinity(), -1}; }

template <typename T>
void block(const PairEnergyArgs& a, int p, int b, Bound<T>& c) {
  typedef stub::W4<T> V;
  const V* src = (const V*)a.src;
  const V* vsrc = (const V*)a.vsrc;
  const auto [me, i] = stub::query_of<T>(a, p);   // the rows form: row first + p, which leaves itself out
  const int j = stub::candidate(a.n_src, me.w, b).j;
  if (j == i) return;
  const T e = stub::absdiff(src[j].x, me.x) - stub::absdiff(vsrc[j].x, vsrc[i].x) - (T)3;
  if (e < c.e) { c.e = e; c.idx = j; }
}

template <typename T>
void store(const PairEnergyArgs& a, int p, const Bound<T>& c) {
  if (a.e) ((T*)a.e)[p] = c.e;
  if (a.idx) a.idx[p] = c.idx;
}

template <typename T>
void pair_energy(const PairEnergyArgs& a) {
  stub::for_each_chunk(a, [&](int p, int y, int b0, int b1) {
    Bound<T> c = none<T>();
    for (int b = b0; b < b1; ++b) block<T>(a, p, b, c);
    if (a.scratch) {
      const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
      ((T*)scratch_e(a))[w] = c.e;
      scratch_idx(a, sizeof(T))[w] = c.idx;
    } else {
      store<T>(a, p, c);
    }
  });
}

template <typename T>
void combine(const PairEnergyArgs& a) {
  for (int p = 0; p < a.m; ++p) {
    Bound<T> c = none<T>();
    for (int y = 0; y < a.chunks; ++y) {
      const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
      const T e = ((const T*)scratch_e(a))[w];
      if (e < c.e) { c.e = e; c.idx = scratch_idx(a, sizeof(T))[w]; }
    }
    store<T>(a, p, c);
  }
}

}  // namespace

namespace nbl {
int launch_pair_energy_kernel(int fp64, hipStream_t, const nbpe::PairEnergyArgs& a) {
  if (nbpe::bad_pair_energy_launch(a)) return (int)hipErrorInvalidValue;
  if (fp64) pair_energy<double>(a); else pair_energy<float>(a);
  return 0;
}
int launch_pair_energy_combine_kernel(int fp64, hipStream_t, const nbpe::PairEnergyArgs& a) {
  if (nbpe::bad_pair_energy_combine(a)) return (int)hipErrorInvalidValue;
  if (fp64) combine<double>(a); else combine<float>(a);
  return 0;
}
}  // namespace nbl
