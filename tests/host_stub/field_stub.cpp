// field_stub.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): a host-only stand-in for the launch functions of field.hip,
// linked beside hip_stub.cpp so that field.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.  hip_stub.cpp's streams
// are synchronous and the field pass is never captured, so both functions execute at launch.
// The stand-in pushes values a test can predict through the REAL FieldArgs — chunk bounds, the per-block scratch layout, the combine's
// ascending sum, pointers the host offset per local and per batch — so ASan sees every offset the host computed.  Per point p and block b
// (T = the context precision; sk = skip[p], or -1 without a skip array):
//   ax_b = src[first source of b].x - x_p     ay_b = y_p + b     az_b = sk (+ src[N - 1].x in the last block)     s_b = w_p
// w_p, which the real kernel ignores, lets a driver tag a point with its index in the caller's array.  accel = (T){sums over b}, w = 0;
// phi = (T)(0 - sum of s_b).  It says nothing about the kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../mini_nbody_amd/csrc/field_args.hpp"

namespace {

template <typename T>
struct W4 { T x, y, z, w; };

template <typename T>
void block_sums(const nbf::FieldArgs& a, int p, int b, T out[4]) {
  typedef W4<T> V;
  const V* src = (const V*)a.src;
  const V me = ((const V*)a.points)[p];
  const int sk = a.skip ? a.skip[p] : -1;
  out[0] = src[(size_t)b * nbd::kSrcBlock].x - me.x;
  out[1] = me.y + (T)b;
  out[2] = (T)sk + (b == a.n_blocks - 1 ? src[a.n_src - 1].x : (T)0);
  out[3] = me.w;
}

template <typename T>
void store_out(const nbf::FieldArgs& a, int p, const double l2[4]) {
  typedef W4<T> V;
  if (a.accel) ((V*)a.accel)[p] = V{(T)l2[0], (T)l2[1], (T)l2[2], (T)0};
  if (a.phi) ((T*)a.phi)[p] = (T)(0.0 - l2[3]);
}

template <typename T>
void field(const nbf::FieldArgs& a, int chunks) {
  T* sc = (T*)a.scratch;
  for (int p = 0; p < a.m; ++p) {
    double l2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int y = 0; y < chunks; ++y) {
      const int blk1 = std::min((y + 1) * a.chunk_blocks, a.n_blocks);
      for (int b = y * a.chunk_blocks; b < blk1; ++b) {
        T s[4];
        block_sums<T>(a, p, b, s);
        for (int q = 0; q < 4; ++q) {
          if (sc) sc[((size_t)b * 4 + q) * (size_t)a.m + (size_t)p] = s[q];
          else l2[q] += (double)s[q];
        }
      }
    }
    if (!sc) store_out<T>(a, p, l2);
  }
}

template <typename T>
void combine(const nbf::FieldArgs& a) {
  const T* sc = (const T*)a.scratch;
  for (int p = 0; p < a.m; ++p) {
    double l2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < a.n_blocks; ++b)
      for (int q = 0; q < 4; ++q) l2[q] += (double)sc[((size_t)b * 4 + q) * (size_t)a.m + (size_t)p];
    store_out<T>(a, p, l2);
  }
}

}  // namespace

namespace nbl {
int launch_field_kernel(int fp64, int, hipStream_t, int chunks, const nbf::FieldArgs& a) {
  if (a.m <= 0 || chunks < 1 || (chunks > 1 && !a.scratch)) return (int)hipErrorInvalidValue;
  if (fp64) field<double>(a, chunks); else field<float>(a, chunks);
  return 0;
}
int launch_field_combine_kernel(int fp64, hipStream_t, const nbf::FieldArgs& a) {
  if (a.m <= 0 || !a.scratch) return (int)hipErrorInvalidValue;
  if (fp64) combine<double>(a); else combine<float>(a);
  return 0;
}
}  // namespace nbl
