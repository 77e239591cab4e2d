// fof_stub.cpp — TEST INFRASTRUCTURE (tests/test_host_sanitizers.py): a host-only stand-in for the launch functions of fof.hip,
// linked beside hip_stub.cpp so that fof.cpp runs on a machine without a GPU under AddressSanitizer / UBSan.  hip_stub.cpp's streams
// are synchronous and the pass is never captured, so both functions execute at launch.
// The stand-in computes the REAL m of include/nbody.h — per row the lowest foreign label among the bodies with d2 <= b2 — from the REAL
// FofArgs: the row's body from a.rows or a.first, the labels from a.label, chunk bounds, the chunks' scratch layout [chunk][m], the
// combine's minimum, pointers the host offset per local and per batch, so ASan sees every offset the host computed.  d2 is the plain
// sum of the three squared differences: the driver's bodies sit on small integers, where every form of it is exact.  It says nothing
// about the kernels' arithmetic (the GPU tests do).
#include <hip/hip_runtime.h>

#include "../../mini_nbody_amd/csrc/fof_args.hpp"
#include "stub_common.hpp"

namespace {

using namespace nbg;

template <typename T>
void link(const FofArgs& a) {
  typedef stub::W4<T> V;
  const V* src = (const V*)a.src;
  const T b2 = (T)a.b2;
  for (int p = 0; p < a.m; ++p) {
    const int i = a.rows ? a.rows[p] : a.first + p;
    const V me = src[i];
    const int mine = a.label[i];
    for (int y = 0; y < a.chunks; ++y) {
      const int s0 = y * a.chunk_blocks * nbd::kSrcBlock;
      const int s1 = std::min(std::min((y + 1) * a.chunk_blocks, a.n_blocks) * nbd::kSrcBlock, a.n_src);
      int m = kFoNone;
      for (int j = s0; j < s1; ++j) {
        const T dx = src[j].x - me.x, dy = src[j].y - me.y, dz = src[j].z - me.z;
        if (dx * dx + dy * dy + dz * dz <= b2 && a.label[j] != mine) m = std::min(m, a.label[j]);
      }
      if (a.scratch) a.scratch[(size_t)y * (size_t)a.m + (size_t)p] = m;
      else a.out[p] = m;
    }
  }
}

}  // namespace

// combine launches so far (one per batch of a split launch), rows walked so far, and how many of them came from an active-row list
STUB_COUNTER(fof_stub_combines)
STUB_COUNTER(fof_stub_rows)
STUB_COUNTER(fof_stub_listed)

namespace nbl {
int launch_fof_kernel(int fp64, hipStream_t, const nbg::FofArgs& a) {
  if (nbg::bad_fof_launch(a)) return (int)hipErrorInvalidValue;
  // the stub's own: what the host promises beyond the guard (the block count, a linking length that is no NaN, ascending rows in range)
  if (a.n_blocks != (a.n_src + nbd::kSrcBlock - 1) / nbd::kSrcBlock || !(a.b2 >= 0.0)) return (int)hipErrorInvalidValue;
  if (a.rows)
    for (int p = 0; p < a.m; ++p)
      if (a.rows[p] < 0 || a.rows[p] >= a.n_src || (p > 0 && a.rows[p] <= a.rows[p - 1])) return (int)hipErrorInvalidValue;
  g_fof_stub_rows.fetch_add(a.m);
  if (a.rows) g_fof_stub_listed.fetch_add(a.m);
  if (fp64) link<double>(a); else link<float>(a);
  return 0;
}
int launch_fof_combine_kernel(hipStream_t, const nbg::FofArgs& a) {
  if (nbg::bad_fof_combine(a)) return (int)hipErrorInvalidValue;
  g_fof_stub_combines.fetch_add(1);
  for (int p = 0; p < a.m; ++p) {
    int m = nbg::kFoNone;
    for (int y = 0; y < a.chunks; ++y) m = std::min(m, a.scratch[(size_t)y * (size_t)a.m + (size_t)p]);
    a.out[p] = m;
  }
  return 0;
}
}  // namespace nbl
