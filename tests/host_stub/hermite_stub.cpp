// hermite_stub.cpp — TEST INFRASTRUCTURE (tests/test_hermite_host_sanitizers.py): a host-only stand-in for the launch functions of
// hermite.hip, linked beside hip_stub.cpp and jerk_stub.cpp (which stands in for the jerk pass the step evaluates with) so that
// hermite.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.  hip_stub.cpp's streams are synchronous, so every
// function executes at launch.
// The stand-in pushes the step's own arithmetic (hermite_args.hpp) through the REAL HermiteArgs — the own slice's offset into pos[cur],
// the saved words, both sets of (a, j) words, the coefficients of either precision — so ASan sees every pointer the host computed, and
// refuses what the real launch functions refuse, by the same predicates.  The best-row reduction is the plain ascending scan with
// strict <, which is what the two-level form on the device amounts to.  It says nothing about the kernels themselves (the GPU tests do).
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "../../mini_nbody_amd/csrc/hermite_args.hpp"
#include "stub_common.hpp"

namespace {

using nbh::BestRatio;
using nbh::Coefficients;
using nbh::HermiteArgs;
using stub::W4;

template <typename T> Coefficients<T> coefficients(const HermiteArgs& a);
template <> Coefficients<float> coefficients<float>(const HermiteArgs& a) { return {a.h, a.c2, a.c3, a.hh, a.c12}; }
template <> Coefficients<double> coefficients<double>(const HermiteArgs& a) { return {a.h_d, a.c2_d, a.c3_d, a.hh_d, a.c12_d}; }

template <typename T>
void predict(const HermiteArgs& a) {
  typedef W4<T> V;
  const Coefficients<T> c = coefficients<T>(a);
  for (int p = 0; p < a.rows; ++p) {
    const V x0 = ((const V*)a.pos)[p], v0 = ((const V*)a.vel)[p], a0 = ((const V*)a.a0)[p], j0 = ((const V*)a.j0)[p];
    ((V*)a.pos0)[p] = x0;
    ((V*)a.vel0)[p] = v0;
    V xp = x0, vp = v0;
    xp.x = std::fma(c.c3, j0.x, std::fma(c.c2, a0.x, std::fma(c.h, v0.x, x0.x)));
    xp.y = std::fma(c.c3, j0.y, std::fma(c.c2, a0.y, std::fma(c.h, v0.y, x0.y)));
    xp.z = std::fma(c.c3, j0.z, std::fma(c.c2, a0.z, std::fma(c.h, v0.z, x0.z)));
    vp.x = std::fma(c.c2, j0.x, std::fma(c.h, a0.x, v0.x));
    vp.y = std::fma(c.c2, j0.y, std::fma(c.h, a0.y, v0.y));
    vp.z = std::fma(c.c2, j0.z, std::fma(c.h, a0.z, v0.z));
    ((V*)a.pos)[p] = xp;
    ((V*)a.vel)[p] = vp;
  }
}

template <typename T>
T corrected_v(const Coefficients<T>& c, T v0, T a0, T a1, T j0, T j1) {
  const T dj = j0 - j1, sa = a0 + a1;
  return std::fma(c.c12, dj, std::fma(c.hh, sa, v0));
}
template <typename T>
T corrected_x(const Coefficients<T>& c, T x0, T v0, T v1, T a0, T a1) {
  const T da = a0 - a1, sv = v0 + v1;
  return std::fma(c.c12, da, std::fma(c.hh, sv, x0));
}

template <typename T>
void correct(const HermiteArgs& a) {
  typedef W4<T> V;
  const Coefficients<T> c = coefficients<T>(a);
  for (int p = 0; p < a.rows; ++p) {
    const V x0 = ((const V*)a.pos0)[p], v0 = ((const V*)a.vel0)[p];
    const V a0 = ((const V*)a.a0)[p], j0 = ((const V*)a.j0)[p], a1 = ((const V*)a.a1)[p], j1 = ((const V*)a.j1)[p];
    V x1 = x0, v1 = v0;
    v1.x = corrected_v(c, v0.x, a0.x, a1.x, j0.x, j1.x);
    v1.y = corrected_v(c, v0.y, a0.y, a1.y, j0.y, j1.y);
    v1.z = corrected_v(c, v0.z, a0.z, a1.z, j0.z, j1.z);
    x1.x = corrected_x(c, x0.x, v0.x, v1.x, a0.x, a1.x);
    x1.y = corrected_x(c, x0.y, v0.y, v1.y, a0.y, a1.y);
    x1.z = corrected_x(c, x0.z, v0.z, v1.z, a0.z, a1.z);
    ((V*)a.pos)[p] = x1;
    ((V*)a.vel)[p] = v1;
  }
}

template <typename T>
void best(const W4<T>* acc, const W4<T>* jerk, int rows, int first, BestRatio* out) {
  BestRatio b = {std::numeric_limits<double>::infinity(), -1, 0};
  for (int r = 0; r < rows; ++r) {
    const double ax = (double)acc[r].x, ay = (double)acc[r].y, az = (double)acc[r].z;
    const double jx = (double)jerk[r].x, jy = (double)jerk[r].y, jz = (double)jerk[r].z;
    const double a2 = (ax * ax + ay * ay) + az * az, j2 = (jx * jx + jy * jy) + jz * jz;
    const double q = a2 / j2;
    if (q < b.q) { b.q = q; b.row = first + r; }
  }
  *out = b;
}

}  // namespace

namespace nbl {
int launch_hermite_predict_kernel(int fp64, hipStream_t, const HermiteArgs& a) {
  if (nbh::bad_hermite_predict(a)) return (int)hipErrorInvalidValue;
  if (fp64) predict<double>(a); else predict<float>(a);
  return 0;
}
int launch_hermite_correct_kernel(int fp64, hipStream_t, const HermiteArgs& a) {
  if (nbh::bad_hermite_correct(a)) return (int)hipErrorInvalidValue;
  if (fp64) correct<double>(a); else correct<float>(a);
  return 0;
}
int launch_hermite_best_kernel(int fp64, hipStream_t, const void* accel, const void* jerk, int rows, int first, BestRatio* out) {
  if (nbd::bad_row_reduce(rows, out, accel && jerk)) return (int)hipErrorInvalidValue;
  if (fp64) best<double>((const W4<double>*)accel, (const W4<double>*)jerk, rows, first, out);
  else best<float>((const W4<float>*)accel, (const W4<float>*)jerk, rows, first, out);
  return 0;
}
}  // namespace nbl
