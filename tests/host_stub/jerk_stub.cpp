// jerk_stub.cpp — TEST INFRASTRUCTURE (tests/test_jerk_host_sanitizers.py): a host-only stand-in for the launch functions of
// point_sums.hip that knows all three passes, linked beside hip_stub.cpp so that point_sums.cpp runs on a machine without a GPU under
// AddressSanitizer / UBSan.  (point_sums_stub.cpp stores a pass it does not know as the field's and reads neither velocity pointer, so
// it cannot serve the jerk; the field's and the tidal's values here are its values.)  hip_stub.cpp's streams are synchronous and no pass
// is ever captured, so both functions execute at launch.
// The stand-in pushes values a test can predict through the REAL PointSumsArgs — chunk bounds, the per-block scratch layout, the
// combine's ascending sum, pointers the host offset per local and per batch, BOTH velocity pointers and the rows form's offset into
// src / vsrc — so ASan sees every offset the host computed.  Per query p and block b (T = the context precision):
//   field, tidal   q0_b = src[first source of b].x - x_p   q1_b = y_p + b   q2_b = sk (+ src[N - 1].x in the last block)   q3_b = w_p
//                  q4_b = b   q5_b = 1   q6_b = z_p       (field: the first four, tidal: all; sk = skip[p], or -1 without a skip array)
//   jerk           (me, mv) = (points[p], pvel[p]) and sk = skip[p] or -1 — or, in the rows form, (src[first + p], vsrc[first + p]) and
//                  sk = first + p:
//                  q0_b = src[first source of b].x - me.x      q1_b = vsrc[first source of b].x - mv.x
//                  q2_b = sk (+ src[N - 1].x in the last block)   q3_b = mv.y (+ vsrc[N - 1].x in the last block)
//                  q4_b = me.w                                 q5_b = mv.w
// The w words, which the real kernel ignores, let a driver tag a query with its index in the caller's arrays.  The results are the real
// kernels' of the sums Q over b: field accel = (T){Q0, Q1, Q2}, w = 0, and phi = (T)(0 - Q3); tidal (T)(Q0 - Q6), (T)(Q1 - Q6),
// (T)(Q2 - Q6), (T)Q3, (T)Q4, (T)Q5; jerk accel = (T){Q0, Q1, Q2}, jerk = (T){Q3, Q4, Q5}, w = 0 in both.  It says nothing about the
// kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include "../../mini_nbody_amd/csrc/point_sums_args.hpp"
#include "stub_common.hpp"

namespace {

using nbp::PointPass;
using nbp::PointSumsArgs;
using stub::W4;

constexpr int kMaxSums = 7;

template <typename T>
void block_sums(const PointPass& pass, const PointSumsArgs& a, int p, int b, T out[kMaxSums]) {
  typedef W4<T> V;
  const V* src = (const V*)a.src;
  const bool last = b == a.n_blocks - 1;
  if (pass.id == nbp::kJerkPass.id) {
    const V* vsrc = (const V*)a.vsrc;
    const bool rows = !a.points;
    const V me = rows ? src[a.first + p] : ((const V*)a.points)[p];
    const V mv = rows ? vsrc[a.first + p] : ((const V*)a.pvel)[p];
    const int sk = rows ? a.first + p : a.skip ? a.skip[p] : -1;
    out[0] = src[(size_t)b * nbd::kSrcBlock].x - me.x;
    out[1] = vsrc[(size_t)b * nbd::kSrcBlock].x - mv.x;
    out[2] = (T)sk + (last ? src[a.n_src - 1].x : (T)0);
    out[3] = mv.y + (last ? vsrc[a.n_src - 1].x : (T)0);
    out[4] = me.w;
    out[5] = mv.w;
    out[6] = (T)0;
    return;
  }
  const V me = ((const V*)a.points)[p];
  const int sk = a.skip ? a.skip[p] : -1;
  out[0] = src[(size_t)b * nbd::kSrcBlock].x - me.x;
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
  } else if (pass.id == nbp::kJerkPass.id) {
    if (a.out[0]) ((V*)a.out[0])[p] = V{(T)l2[0], (T)l2[1], (T)l2[2], (T)0};
    if (a.out[1]) ((V*)a.out[1])[p] = V{(T)l2[3], (T)l2[4], (T)l2[5], (T)0};
  } else {
    if (a.out[0]) ((V*)a.out[0])[p] = V{(T)l2[0], (T)l2[1], (T)l2[2], (T)0};
    if (a.out[1]) ((T*)a.out[1])[p] = (T)(0.0 - l2[3]);
  }
}

template <typename T>
void sums(const PointPass& pass, const PointSumsArgs& a, int chunks) {
  T* sc = (T*)a.scratch;
  for (int p = 0; p < a.m; ++p) {
    double l2[kMaxSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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
    double l2[kMaxSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < a.n_blocks; ++b)
      for (int q = 0; q < pass.sums; ++q) l2[q] += (double)sc[((size_t)b * pass.sums + q) * (size_t)a.m + (size_t)p];
    store_out<T>(pass, a, p, l2);
  }
}

}  // namespace

namespace nbl {
int launch_point_sums_kernel(const PointPass& pass, int fp64, int, hipStream_t, int chunks, const PointSumsArgs& a) {
  if (nbp::bad_point_sums_launch(a, chunks) || nbp::bad_point_sums_queries(pass, a)) return (int)hipErrorInvalidValue;
  if (fp64) sums<double>(pass, a, chunks); else sums<float>(pass, a, chunks);
  return 0;
}
int launch_point_sums_combine_kernel(const PointPass& pass, int fp64, hipStream_t, const PointSumsArgs& a) {
  if (nbp::bad_point_sums_combine(a)) return (int)hipErrorInvalidValue;
  if (fp64) combine<double>(pass, a); else combine<float>(pass, a);
  return 0;
}
}  // namespace nbl
