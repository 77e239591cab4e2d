// hermite_args.hpp — what hermite.cpp (host) and hermite.hip (device) agree on: the argument block of the Hermite step's two elementwise
// kernels, the word of the a^2 / j^2 best-row reduction and the launch functions of hermite.hip.  Like timescale_args.hpp it stays apart
// from nbody_args.hpp, the force path's hashed kernel source.
//
// The step (include/nbody.h, "fourth-order Hermite integrator") in the context precision T, every operation rounded once, products fused
// only where fma is written, with h = dt and the coefficients computed once per step on the host in T (coefficients_of below):
//   predict   xp = fma(c3, j0, fma(c2, a0, fma(h, v0, x0)))      vp = fma(c2, j0, fma(h, a0, v0))
//   correct   v1 = fma(c12, j0 - j1, fma(hh, a0 + a1, v0))      x1 = fma(c12, a0 - a1, fma(hh, v0 + v1, x0))
// per component; the position word's w and the velocity word's fourth value are carried bit for bit.  The all-pairs work between the two
// is the jerk rows pass of point_sums.hip over the predicted state.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbh {

// the coefficients of a step of h, in T: h2 = h * h, c2 = h2 * 0.5, c3 = (h2 * h) / 6, hh = h * 0.5, c12 = h2 / 12 (IEEE quotients).
// Host and device: the shared step forms them once on the host, the block step (hermite_block.hip) per row on the device, where the
// plain / of a file compiled with contraction off is the correctly rounded quotient too (timescale.hip relies on the same).
template <typename T>
struct Coefficients { T h, c2, c3, hh, c12; };
template <typename T>
__host__ __device__ inline Coefficients<T> coefficients_of(T h) {
  const T h2 = h * h;   // (products and quotients only: nothing here can be contracted)
  return {h, h2 * (T)0.5, (h2 * h) / (T)6, h * (T)0.5, h2 / (T)12};
}

struct HermiteArgs {
  void* pos;         // [rows] position words of the local's own slice (16-B or 32-B {x, y, z, w}): predict reads x0 and writes xp, correct writes x1
  void* vel;         // [rows] velocity words of the local's own slice: predict reads v0 and writes vp, correct writes v1
  void* pos0;        // [rows] x0 words: predict writes them, correct reads them
  void* vel0;        // [rows] v0 words likewise
  const void* a0;    // [rows] words {ax, ay, az, 0} and ...
  const void* j0;    // ... {jx, jy, jz, 0} at the start of the step
  const void* a1;    // the same at the predicted state: correct only (predict leaves them null)
  const void* j1;
  int rows;
  float h, c2, c3, hh, c12;          // the coefficients of an fp32 context ...
  double h_d, c2_d, c3_d, hh_d, c12_d;   // ... and of an fp64 one
};

// what the two launches refuse
inline bool bad_hermite_predict(const HermiteArgs& a) { return a.rows <= 0 || !a.pos || !a.vel || !a.pos0 || !a.vel0 || !a.a0 || !a.j0; }
inline bool bad_hermite_correct(const HermiteArgs& a) { return bad_hermite_predict(a) || !a.a1 || !a.j1; }

// q of a row in binary64 from the T values: a2 = (ax ax + ay ay) + az az, j2 likewise, q = a2 / j2 (0 / 0 = NaN, a2 / 0 = +inf)
template <typename V4>
__host__ __device__ inline double ratio_of(const V4 a, const V4 j) {
  const double ax = (double)a.x, ay = (double)a.y, az = (double)a.z, jx = (double)j.x, jy = (double)j.y, jz = (double)j.z;
  const double a2 = (ax * ax + ay * ay) + az * az;
  const double j2 = (jx * jx + jy * jy) + jz * jz;
  return a2 / j2;
}

// what hermite_best leaves per device or rank: the smallest q = a2 / j2 of its rows (binary64, from the T values) with the lowest global
// row that reaches it; row < 0: no candidate, q = +inf
struct BestRatio { double q; int row, pad; };

}  // namespace nbh

namespace nbl {
// all return a hipError_t as int (0 = launched).  grid = ceil(rows / nbd::kLanes), one row per lane
int launch_hermite_predict_kernel(int fp64, hipStream_t stream, const nbh::HermiteArgs& a);
int launch_hermite_correct_kernel(int fp64, hipStream_t stream, const nbh::HermiteArgs& a);
// the best of `rows` rows' q_r = |accel[r]|^2 / |jerk[r]|^2 in binary64, row r being global body first + r: smallest q, then lowest row;
// a NaN or +inf q is never chosen.  One workgroup, a fixed order
int launch_hermite_best_kernel(int fp64, hipStream_t stream, const void* accel, const void* jerk, int rows, int first, nbh::BestRatio* out);
}  // namespace nbl
