// timescale_stub.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py, case `timescale`): a host-only stand-in for the launch functions of
// timescale.hip, linked beside hip_stub.cpp so that timescale.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.
// hip_stub.cpp's streams are synchronous and the pass is never captured, so all three functions execute at launch.
// The stand-in pushes values a test can predict through the REAL TimescaleArgs — chunk bounds, the chunks' scratch layout, the combine's
// ascending strict <, pointers the host offset per local and per batch, the rows' first, and BOTH source streams — so ASan sees every
// offset the host computed and a driver sees whether all N velocities arrived.  Per row p (i = first + p, me = src[i], mv = vsrc[i])
// every block b offers the ONE candidate j_b of stub_rule.hpp (steered by me.w; none if j_b == i), of which the stub takes
//   q_b = |src[j_b].x - me.x|      d2_b = |vsrc[j_b].x - mv.x|
// in ascending b with strict < for both minima.  It says nothing about the kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include <limits>

#include "../../mini_nbody_amd/csrc/timescale_args.hpp"
#include "stub_common.hpp"

namespace {

using namespace nbts;

template <typename T>
struct Scale { T tau2; int idx; T d2min; };

template <typename T>
Scale<T> none() { return {std::numeric_limits<T>::infinity(), -1, std::numeric_limits<T>::infinity()}; }

template <typename T>
void block(const TimescaleArgs& a, int p, int b, Scale<T>& c) {
  typedef stub::W4<T> V;
  const V* src = (const V*)a.src;
  const V* vsrc = (const V*)a.vsrc;
  const auto [me, i] = stub::query_of<T>(a, p);   // the rows form: row first + p, which leaves itself out
  const int j = stub::candidate(a.n_src, me.w, b).j;
  if (j == i) return;
  const T q = stub::absdiff(src[j].x, me.x), d2 = stub::absdiff(vsrc[j].x, vsrc[i].x);
  if (q < c.tau2) { c.tau2 = q; c.idx = j; }
  if (d2 < c.d2min) c.d2min = d2;
}

template <typename T>
void store(const TimescaleArgs& a, int p, const Scale<T>& c) {
  if (a.tau2) ((T*)a.tau2)[p] = c.tau2;
  if (a.idx) a.idx[p] = c.idx;
  if (a.d2min) ((T*)a.d2min)[p] = c.d2min;
}

template <typename T>
void timescale(const TimescaleArgs& a) {
  stub::for_each_chunk(a, [&](int p, int y, int b0, int b1) {
    Scale<T> c = none<T>();
    for (int b = b0; b < b1; ++b) block<T>(a, p, b, c);
    if (a.scratch) {
      const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
      ((T*)scratch_tau2(a))[w] = c.tau2;
      ((T*)scratch_d2(a, sizeof(T)))[w] = c.d2min;
      scratch_idx(a, sizeof(T))[w] = c.idx;
    } else {
      store<T>(a, p, c);
    }
  });
}

template <typename T>
void combine(const TimescaleArgs& a) {
  for (int p = 0; p < a.m; ++p) {
    Scale<T> c = none<T>();
    for (int y = 0; y < a.chunks; ++y) {
      const size_t w = (size_t)y * (size_t)a.m + (size_t)p;
      const T q = ((const T*)scratch_tau2(a))[w], d2 = ((const T*)scratch_d2(a, sizeof(T)))[w];
      if (q < c.tau2) { c.tau2 = q; c.idx = scratch_idx(a, sizeof(T))[w]; }
      if (d2 < c.d2min) c.d2min = d2;
    }
    store<T>(a, p, c);
  }
}

template <typename T>
void best(const T* tau2, const int* idx, const T* d2min, int rows, int first, BestScale* out) {
  const double inf = std::numeric_limits<double>::infinity();
  BestScale b = {inf, inf, -1, -1};
  for (int r = 0; r < rows; ++r) {
    if ((double)tau2[r] < b.tau2) { b.tau2 = (double)tau2[r]; b.i = first + r; b.j = idx[r]; }
    if ((double)d2min[r] < b.d2min) b.d2min = (double)d2min[r];
  }
  *out = b;
}

}  // namespace

namespace nbl {
int launch_timescale_kernel(int fp64, hipStream_t, const nbts::TimescaleArgs& a) {
  if (nbts::bad_timescale_launch(a)) return (int)hipErrorInvalidValue;
  if (fp64) timescale<double>(a); else timescale<float>(a);
  return 0;
}
int launch_timescale_combine_kernel(int fp64, hipStream_t, const nbts::TimescaleArgs& a) {
  if (nbd::bad_combine(a)) return (int)hipErrorInvalidValue;
  if (fp64) combine<double>(a); else combine<float>(a);
  return 0;
}
int launch_timescale_best_kernel(int fp64, hipStream_t, const void* tau2, const int* idx, const void* d2min, int rows, int first,
                                 nbts::BestScale* out) {
  if (nbd::bad_row_reduce(rows, out, tau2 && idx && d2min)) return (int)hipErrorInvalidValue;
  if (fp64) best<double>((const double*)tau2, idx, (const double*)d2min, rows, first, out);
  else best<float>((const float*)tau2, idx, (const float*)d2min, rows, first, out);
  return 0;
}
}  // namespace nbl
