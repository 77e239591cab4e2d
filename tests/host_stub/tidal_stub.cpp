// tidal_stub.cpp — TEST INFRASTRUCTURE (tests/test_tidal_host_sanitizers.py): a host-only stand-in for the launch functions of
// tidal.hip, linked beside hip_stub.cpp so that tidal.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.
// hip_stub.cpp's streams are synchronous and the tidal pass is never captured, so both functions execute at launch.
// The stand-in pushes values a test can predict through the REAL TidalArgs — chunk bounds, the per-block scratch layout, the combine's
// ascending sum, pointers the host offset per local and per batch — so ASan sees every offset the host computed.  Per point p and block b
// (T = the context precision; sk = skip[p], or -1 without a skip array), the seven level-1 sums:
//   q0_b = src[first source of b].x - x_p   q1_b = y_p + b   q2_b = sk (+ src[N - 1].x in the last block)   q3_b = w_p   q4_b = b
//   q5_b = 1   s3_b = z_p
// w_p, which the real kernel ignores, lets a driver tag a point with its index in the caller's array.  The six values are the real
// kernel's: (T)(Q0 - S3), (T)(Q1 - S3), (T)(Q2 - S3), (T)Q3, (T)Q4, (T)Q5 of the sums over b.  It says nothing about the kernels'
// arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../mini_nbody_amd/csrc/tidal_args.hpp"

namespace {

using nbt::kOut;
using nbt::kSums;

template <typename T>
struct W4 { T x, y, z, w; };

template <typename T>
void block_sums(const nbt::TidalArgs& a, int p, int b, T out[kSums]) {
  typedef W4<T> V;
  const V* src = (const V*)a.src;
  const V me = ((const V*)a.points)[p];
  const int sk = a.skip ? a.skip[p] : -1;
  out[0] = src[(size_t)b * nbd::kSrcBlock].x - me.x;
  out[1] = me.y + (T)b;
  out[2] = (T)sk + (b == a.n_blocks - 1 ? src[a.n_src - 1].x : (T)0);
  out[3] = me.w;
  out[4] = (T)b;
  out[5] = (T)1;
  out[6] = me.z;
}

template <typename T>
void store_out(const nbt::TidalArgs& a, int p, const double l2[kSums]) {
  T* out = (T*)a.tensor + (size_t)p * kOut;
  for (int q = 0; q < 3; ++q) out[q] = (T)(l2[q] - l2[6]);
  for (int q = 3; q < kOut; ++q) out[q] = (T)l2[q];
}

template <typename T>
void tidal(const nbt::TidalArgs& a, int chunks) {
  T* sc = (T*)a.scratch;
  for (int p = 0; p < a.m; ++p) {
    double l2[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int y = 0; y < chunks; ++y) {
      const int blk1 = std::min((y + 1) * a.chunk_blocks, a.n_blocks);
      for (int b = y * a.chunk_blocks; b < blk1; ++b) {
        T s[kSums];
        block_sums<T>(a, p, b, s);
        for (int q = 0; q < kSums; ++q) {
          if (sc) sc[((size_t)b * kSums + q) * (size_t)a.m + (size_t)p] = s[q];
          else l2[q] += (double)s[q];
        }
      }
    }
    if (!sc) store_out<T>(a, p, l2);
  }
}

template <typename T>
void combine(const nbt::TidalArgs& a) {
  const T* sc = (const T*)a.scratch;
  for (int p = 0; p < a.m; ++p) {
    double l2[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < a.n_blocks; ++b)
      for (int q = 0; q < kSums; ++q) l2[q] += (double)sc[((size_t)b * kSums + q) * (size_t)a.m + (size_t)p];
    store_out<T>(a, p, l2);
  }
}

}  // namespace

namespace nbl {
int launch_tidal_kernel(int fp64, int, hipStream_t, int chunks, const nbt::TidalArgs& a) {
  if (a.m <= 0 || chunks < 1 || (chunks > 1 && !a.scratch) || !a.tensor) return (int)hipErrorInvalidValue;
  if (fp64) tidal<double>(a, chunks); else tidal<float>(a, chunks);
  return 0;
}
int launch_tidal_combine_kernel(int fp64, hipStream_t, const nbt::TidalArgs& a) {
  if (a.m <= 0 || !a.scratch || !a.tensor) return (int)hipErrorInvalidValue;
  if (fp64) combine<double>(a); else combine<float>(a);
  return 0;
}
}  // namespace nbl
