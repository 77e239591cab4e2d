// mutual_stub.cpp — TEST INFRASTRUCTURE (tests/test_mutual_host_sanitizers.py): hip_stub.cpp as it is, and a stand-in for the launch
// function of mutual.hip that runs the REAL MutualArgs through the data flow of the launch, so that mutual.cpp (which passes take the
// mutual pairing, the table, the counters) runs on a machine without a GPU under AddressSanitizer / UBSan.  The stand-in force is
// hip_stub.cpp's (F_i = sum of (r_j - r_i)): T[source block][row] = the row against the block, every unit of the library's own
// enumeration walked, and the program ABORTS if a word of the table is written twice or never, or a counter is not zero when the launch
// begins; then the rows are folded as the kernel folds them (blocks of a piece, pieces of a segment, segments, ascending) and applied.
// It says nothing about the kernel's arithmetic (the GPU tests do).  Linked INSTEAD of hip_stub.cpp, which it includes.
#include "hip_stub.cpp"

#include "../../mini_nbody_amd/csrc/mutual_args.hpp"

namespace {

long g_mutual_launches = 0;

void mutual_launch(const nbm::MutualArgs& a) {
  typedef W4<float> V;
  const V* src = (const V*)a.src;
  V* table = (V*)a.table;
  for (int x = 0; x < a.nb; ++x) if (a.tickets[x] != 0) abort();
  std::vector<char> written((size_t)a.nb * a.n, 0);
  for (int u = 0; u < a.nunits; ++u) {
    const nbm::Unit un = nbm::mutual_unit(a.nb, a.run, u);
    for (int k = 0; k < un.count; ++k) {
      const int A = un.a, B = (un.a + un.d0 + k) % a.nb;
      for (int side = 0; side < (un.d0 ? 2 : 1); ++side) {   // rows of A against block B, then (off the diagonal) rows of B against block A
        const int R = side ? B : A, S = side ? A : B;
        for (int i = R * nbm::kBlock; i < (R + 1) * nbm::kBlock; ++i) {
          V t = {0, 0, 0, 0};
          for (int j = S * nbm::kBlock; j < (S + 1) * nbm::kBlock; ++j) { t.x += src[j].x - src[i].x; t.y += src[j].y - src[i].y; t.z += src[j].z - src[i].z; }
          const size_t at = (size_t)S * a.n + i;
          if (written[at]++) abort();   // a block pair taken twice
          table[at] = t;
        }
        a.tickets[R] += 1;
      }
    }
  }
  for (char w : written) if (!w) abort();   // a block pair never taken
  for (int x = 0; x < a.nb; ++x) { if ((int)a.tickets[x] != a.nb) abort(); a.tickets[x] = 0; }
  for (int i = 0; i < a.f.n_src; ++i) {
    float fx = 0, fy = 0, fz = 0;
    for (int q = 0; q < a.f.nslices; ++q)
      for (int t = 0; t < a.f.sub; ++t) {
        int jb, je;
        nbk::segment_bounds(q, t, a.f.n_src, a.f.nslices, a.f.sub, &jb, &je);
        for (int w = 0; w < a.f.wsplit; ++w) {
          int pb = jb, pe = je;
          if (a.f.wsplit > 1) nbk::piece_bounds(jb, je, w, a.f.wsplit, &pb, &pe);
          if (pb % nbm::kBlock || pe % nbm::kBlock) abort();   // the host let a pass through whose pieces are not whole blocks
          for (int blk = pb / nbm::kBlock; blk < pe / nbm::kBlock; ++blk) { const V e = table[(size_t)blk * a.f.n_src + i]; fx += e.x; fy += e.y; fz += e.z; }
        }
      }
    apply<float>(a.f, i, fx, fy, fz);
  }
}

}  // namespace

extern "C" long mutual_stub_launches(void) { return g_mutual_launches; }

namespace nbl {
int launch_mutual_pairs_kernel(hipStream_t, const nbm::MutualArgs& a) {
  return enqueue([=] { ++g_mutual_launches; mutual_launch(a); });
}
}  // namespace nbl
