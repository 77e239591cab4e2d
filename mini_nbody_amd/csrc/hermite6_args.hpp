// hermite6_args.hpp — what hermite6.cpp (host) and hermite6.hip (device) agree on: the argument block of the sixth-order Hermite step's
// two elementwise kernels and their launch functions.  Like hermite_args.hpp it stays apart from nbody_args.hpp, the force path's hashed
// kernel source; the best-row reduction and its word are hermite_args.hpp's.
//
// The step (include/nbody.h, "sixth-order Hermite integrator"; Nitadori & Makino 2008) in the context precision T, every operation rounded
// once, products fused only where fma is written, with h = dt and the coefficients computed once per step on the host in T
// (coefficients6_of below); (a, j, s) acceleration, jerk and snap, c the crackle (the third derivative of a):
//   predict   xp = fma(c5, c0, fma(c4, s0, fma(c3, j0, fma(c2, a0, fma(h, v0, x0)))))
//             vp = fma(c4, c0, fma(c3, s0, fma(c2, j0, fma(h, a0, v0))))
//             ap = fma(c3, c0, fma(c2, s0, fma(h, j0, a0)))
//   correct   v1 = fma(c120, s0 + s1, fma(c10, j0 - j1, fma(hh, a0 + a1, v0)))
//             x1 = fma(c120, j0 + j1, fma(c10, a0 - a1, fma(hh, v0 + v1, x0)))
//   crackle   e1 = 60 (a1 - a0), e2 = fma(36, j1, 24 j0), e3 = fma(9, s1, -3 s0), c1 = r fma(r, fma(r, e1, -e2), e3): the third
//             derivative of the quintic through (a0, j0, s0) and (a1, j1, s1) at the end of the step, what the next predictor takes as c0
// per component; the position word's w and the velocity word's fourth value are carried bit for bit, the fourth value of ap and c1 is that
// of a0 and a1 (0).  The all-pairs work between the two is the snap rows pass of point_sums.hip over the predicted (xp, vp, ap).
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbh6 {

// the coefficients of a step of h, in T: h2 = h * h, c2 = h2 * 0.5, c3 = (h2 * h) / 6, c4 = (h2 * h2) / 24, c5 = ((h2 * h2) * h) / 120,
// hh = h * 0.5, c10 = h2 / 10, c120 = (h2 * h) / 120, r = 1 / h (IEEE quotients)
template <typename T>
struct Coefficients6 { T h, c2, c3, c4, c5, hh, c10, c120, r; };
template <typename T>
__host__ __device__ inline Coefficients6<T> coefficients6_of(T h) {
  const T h2 = h * h;   // (products and quotients only: nothing here can be contracted)
  return {h, h2 * (T)0.5, (h2 * h) / (T)6, (h2 * h2) / (T)24, ((h2 * h2) * h) / (T)120, h * (T)0.5, h2 / (T)10, (h2 * h) / (T)120, (T)1 / h};
}

struct Hermite6Args {
  void* pos;         // [rows] position words of the local's own slice: predict reads x0 and writes xp, correct writes x1
  void* vel;         // [rows] velocity words of the local's own slice: predict reads v0 and writes vp, correct writes v1
  void* pos0;        // [rows] x0 words: predict writes them, correct reads them
  void* vel0;        // [rows] v0 words likewise
  const void* a0;    // [rows] words {., ., ., 0}: acceleration, ...
  const void* j0;    // ... jerk ...
  const void* s0;    // ... and snap at the start of the step
  void* crk;         // [rows] crackle words: predict reads c0 (zeros in a call's first step), correct writes c1
  void* ap;          // [rows] predicted acceleration words: predict writes them (the snap pass's third source stream)
  const void* a1;    // the three at the predicted state: correct only (predict leaves them null)
  const void* j1;
  const void* s1;
  int rows;
  Coefficients6<float> f;    // the coefficients of an fp32 context ...
  Coefficients6<double> d;   // ... and of an fp64 one
};

// what the two launches refuse
inline bool bad_hermite6_predict(const Hermite6Args& a) {
  return a.rows <= 0 || !a.pos || !a.vel || !a.pos0 || !a.vel0 || !a.a0 || !a.j0 || !a.s0 || !a.crk || !a.ap;
}
inline bool bad_hermite6_correct(const Hermite6Args& a) {
  return a.rows <= 0 || !a.pos || !a.vel || !a.pos0 || !a.vel0 || !a.a0 || !a.j0 || !a.s0 || !a.crk || !a.a1 || !a.j1 || !a.s1;
}

}  // namespace nbh6

namespace nbl {
// both return a hipError_t as int (0 = launched).  grid = ceil(rows / nbd::kLanes), one row per lane
int launch_hermite6_predict_kernel(int fp64, hipStream_t stream, const nbh6::Hermite6Args& a);
int launch_hermite6_correct_kernel(int fp64, hipStream_t stream, const nbh6::Hermite6Args& a);
}  // namespace nbl
