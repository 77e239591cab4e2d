// snap_stub.cpp — TEST INFRASTRUCTURE (tests/test_snap_host_sanitizers.py): a host-only stand-in for the launch functions of
// point_sums.hip that knows all four passes and sizes its sums for the snap's nine, linked beside hip_stub.cpp so that point_sums.cpp
// and hermite6.cpp run on a machine without a GPU under AddressSanitizer / UBSan.  (jerk_stub.cpp sizes its sums for seven and reads no
// acceleration pointer, so it cannot serve the snap; the field's, the tidal's and the jerk's values here are its values.)
// hip_stub.cpp's streams are synchronous and no pass is ever captured, so both functions execute at launch.
// The stand-in pushes values a test can predict through the REAL PointSumsArgs — chunk bounds, the per-block scratch layout, the
// combine's ascending sum, pointers the host offset per local and per batch, ALL THREE source streams, the three point arrays, the rows
// form's offset into src / vsrc / asrc and the third output — so ASan sees every offset the host computed.  Per query p and block b
// (T = the context precision), first = the first source of b, last = the last block:
//   field, tidal   as jerk_stub.cpp states them
//   jerk, snap     (me, mv) = (points[p], pvel[p]) and sk = skip[p] or -1 — or, in the rows form, (src[first + p], vsrc[first + p]) and
//                  sk = first + p:
//                  q0_b = src[first].x - me.x              q1_b = vsrc[first].x - mv.x
//                  q2_b = sk (+ src[N - 1].x in last)      q3_b = mv.y (+ vsrc[N - 1].x in last)
//                  q4_b = me.w                             q5_b = mv.w
//   snap only      ma = pacc[p], or asrc[first + p] in the rows form:
//                  q6_b = asrc[first].x - ma.x             q7_b = ma.y (+ asrc[N - 1].x in last)       q8_b = ma.w
// The results are the real kernels' of the sums Q over b; the snap's: accel = (T){Q0, Q1, Q2}, jerk = (T){Q3, Q4, Q5},
// snap = (T){Q6, Q7, Q8}, w = 0 in all three.  It says nothing about the kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include "../../mini_nbody_amd/csrc/point_sums_args.hpp"
#include "stub_common.hpp"

namespace {

using nbp::PointPass;
using nbp::PointSumsArgs;
using stub::W4;

constexpr int kMaxSums = 9;

template <typename T>
void block_sums(const PointPass& pass, const PointSumsArgs& a, int p, int b, T out[kMaxSums]) {
  typedef W4<T> V;
  const V* src = (const V*)a.src;
  const bool last = b == a.n_blocks - 1;
  const size_t first = (size_t)b * nbd::kSrcBlock;
  for (int q = 0; q < kMaxSums; ++q) out[q] = (T)0;
  if (pass.velocities) {
    const V* vsrc = (const V*)a.vsrc;
    const bool rows = !a.points;
    const V me = rows ? src[a.first + p] : ((const V*)a.points)[p];
    const V mv = rows ? vsrc[a.first + p] : ((const V*)a.pvel)[p];
    const int sk = rows ? a.first + p : a.skip ? a.skip[p] : -1;
    out[0] = src[first].x - me.x;
    out[1] = vsrc[first].x - mv.x;
    out[2] = (T)sk + (last ? src[a.n_src - 1].x : (T)0);
    out[3] = mv.y + (last ? vsrc[a.n_src - 1].x : (T)0);
    out[4] = me.w;
    out[5] = mv.w;
    if (pass.accelerations) {
      const V* asrc = (const V*)a.asrc;
      const V ma = rows ? asrc[a.first + p] : ((const V*)a.pacc)[p];
      out[6] = asrc[first].x - ma.x;
      out[7] = ma.y + (last ? asrc[a.n_src - 1].x : (T)0);
      out[8] = ma.w;
    }
    return;
  }
  const V me = ((const V*)a.points)[p];
  const int sk = a.skip ? a.skip[p] : -1;
  out[0] = src[first].x - me.x;
  out[1] = me.y + (T)b;
  out[2] = (T)sk + (last ? src[a.n_src - 1].x : (T)0);
  out[3] = me.w;
  out[4] = (T)b;
  out[5] = (T)1;
  out[6] = me.z;
}

template <typename T>
void store_out(const PointPass& pass, const PointSumsArgs& a, int p, const double l2[kMaxSums]) {
  typedef W4<T> V;
  if (pass.id == nbp::kTidalPass.id) {
    T* out = (T*)a.out[0] + (size_t)p * pass.out_values[0];
    for (int q = 0; q < 3; ++q) out[q] = (T)(l2[q] - l2[6]);
    for (int q = 3; q < pass.out_values[0]; ++q) out[q] = (T)l2[q];
  } else if (pass.velocities) {
    if (a.out[0]) ((V*)a.out[0])[p] = V{(T)l2[0], (T)l2[1], (T)l2[2], (T)0};
    if (a.out[1]) ((V*)a.out[1])[p] = V{(T)l2[3], (T)l2[4], (T)l2[5], (T)0};
    if (a.out2) ((V*)a.out2)[p] = V{(T)l2[6], (T)l2[7], (T)l2[8], (T)0};
  } else {
    if (a.out[0]) ((V*)a.out[0])[p] = V{(T)l2[0], (T)l2[1], (T)l2[2], (T)0};
    if (a.out[1]) ((T*)a.out[1])[p] = (T)(0.0 - l2[3]);
  }
}

template <typename T>
void sums(const PointPass& pass, const PointSumsArgs& a, int chunks) {
  T* sc = (T*)a.scratch;
  for (int p = 0; p < a.m; ++p) {
    double l2[kMaxSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int y = 0; y < chunks; ++y) {
      const int blk1 = std::min((y + 1) * a.chunk_blocks, a.n_blocks);
      for (int b = y * a.chunk_blocks; b < blk1; ++b) {
        T s[kMaxSums];
        block_sums<T>(pass, a, p, b, s);
        for (int q = 0; q < pass.sums; ++q) {
          if (sc) sc[((size_t)b * pass.sums + q) * (size_t)a.m + (size_t)p] = s[q];
          else l2[q] += (double)s[q];
        }
      }
    }
    if (!sc) store_out<T>(pass, a, p, l2);
  }
}

template <typename T>
void combine(const PointPass& pass, const PointSumsArgs& a) {
  const T* sc = (const T*)a.scratch;
  for (int p = 0; p < a.m; ++p) {
    double l2[kMaxSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < a.n_blocks; ++b)
      for (int q = 0; q < pass.sums; ++q) l2[q] += (double)sc[((size_t)b * pass.sums + q) * (size_t)a.m + (size_t)p];
    store_out<T>(pass, a, p, l2);
  }
}

}  // namespace

namespace nbl {
int launch_point_sums_kernel(const PointPass& pass, int fp64, int, hipStream_t, int chunks, const PointSumsArgs& a) {
  if (pass.sums > kMaxSums || nbp::bad_point_sums_launch(a, chunks) || nbp::bad_point_sums_queries(pass, a)) return (int)hipErrorInvalidValue;
  if (fp64) sums<double>(pass, a, chunks); else sums<float>(pass, a, chunks);
  return 0;
}
int launch_point_sums_combine_kernel(const PointPass& pass, int fp64, hipStream_t, const PointSumsArgs& a) {
  if (pass.sums > kMaxSums || nbp::bad_point_sums_combine(a)) return (int)hipErrorInvalidValue;
  if (fp64) combine<double>(pass, a); else combine<float>(pass, a);
  return 0;
}
}  // namespace nbl
