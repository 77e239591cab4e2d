// stub_rule.hpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): THE contract between the distance passes' stubs (neighbors_stub.cpp,
// knn_stub.cpp, hist_stub.cpp, timescale_stub.cpp), which offer candidates by this rule, and their drivers (*_sanity.cpp), which compute
// the expected values from it.  No HIP include: a driver sees nothing of the library but include/nbody.h.
// Per query with the word {x, y, z, w}, every block b of kBlock sources (len_b of them, from b0_b = kBlock b) offers ONE candidate:
//   j_b = b0_b + ((int)w + b) mod len_b      d2_b = |src[j_b].x - x|      (none if j_b is the excluded body)
// w, which the real kernels ignore, lets a driver steer the candidates.  What a pass makes of the candidates in ascending b — strict <,
// the count rule, the k-list insertion, the cumulative bins, the two minima — is its own fold, stated in its stub and again in its
// driver's expect().
#pragma once
#include <algorithm>

namespace stub {

constexpr int kBlock = 1024;   // = nbd::kSrcBlock (stub_common.hpp asserts it)

template <typename T>
struct W4 { T x, y, z, w; };

template <typename T>
inline T absdiff(T a, T b) { const T d = a - b; return d < 0 ? -d : d; }

inline int blocks_of(int n_src) { return (n_src + kBlock - 1) / kBlock; }

struct Candidate { int j, b0, len; };   // the body block b offers, the block's first source and its length
template <typename T>
inline Candidate candidate(int n_src, T w, int b) {
  const int b0 = b * kBlock, len = std::min(kBlock, n_src - b0);
  return {b0 + ((int)w + b) % len, b0, len};
}

}  // namespace stub
