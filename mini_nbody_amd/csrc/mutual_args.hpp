// mutual_args.hpp — what the host side (mutual.cpp) and the kernels (mutual.hip) of the MUTUAL pairing agree on: the argument blocks, the
// enumeration of the work units and the launch functions.  The mutual pairing (NBODY_OPT_PAIRING = 2) evaluates every unordered pair of
// the fp32 force pass ONCE and returns the bits of the ordered pass of the same configuration:
//   mutual_pairs_f32   the level-1 sums — one chain of 1024 fma per (row, source block), from zero, ascending — of every row against every
//                      source block, each off-diagonal block pair walked once, into the table T[source block][row]; and, by the wave that
//                      writes the last word of a row block, levels 2-4 of the ordered sum restated on the table (blocks of a piece, pieces
//                      of a segment, segments), then apply_force: store, kick, drift
#pragma once
#include "nbody_args.hpp"

namespace nbm {

using nbk::f4;
using nbk::ForceArgs;

constexpr int kBlock = 1024;        // rows of a row block = sources of a level-1 block (NBODY_OPT_SUM_BLOCK must be 1024)
constexpr int kRowsPerLane = 16;    // 64 lanes x 16 rows = one row block per wave
constexpr int kRun = 8;             // source blocks a unit streams past its row block (4 .. 16 measured level, 32 slower: profiles/r18_mutual_pairing.md)
constexpr int kWavesPerWg = 4;      // independent waves: no LDS, no barrier
constexpr int kMaxN = 1 << 26;      // byte offsets inside one table row stay below 2^32

struct MutualArgs {
  ForceArgs f;        // rows, vel, pos_next_rows, force_out, what to apply, and the segmentation of the ORDERED pass: n_src, nslices, sub, wsplit
  const void* src;    // all N = 1024 nb source words, ascending
  f4* table;          // T[source block][row]: nb x N words {Fx, Fy, Fz, 0}; every word written exactly once per pass
  unsigned* tickets;  // table words written so far per row block: nb counters, zero between passes (the wave that completes one zeroes it)
  int n, nb;          // bodies, blocks
  int run;            // partner blocks per unit at most
  int nunits;         // mutual_units(nb, run)
};

// Balanced cyclic pairing: row block A takes the partner blocks A + d (mod nb) for d = 1 .. ceil(nb / 2) - 1, and for even nb also
// d = nb / 2 when A < nb / 2: every unordered pair of blocks once, every A the same work (one block more or less).  The partners of A are cut
// into runs of `run` consecutive d: a unit is (A, first d, count).  The long units come first in launch order; the nb diagonal units
// (A, d = 0, one block, mirrored side off), an eighth as long, come last and fill the launch's tail.
struct Unit { int a, d0, count; };   // count = 0: nothing to do (the run lies beyond this A's last partner)

__device__ __host__ inline int mutual_max_d(int nb) { return (nb + 1) / 2 - 1 + (nb % 2 == 0 ? 1 : 0); }
__device__ __host__ inline int mutual_runs(int nb, int run) { return (mutual_max_d(nb) + run - 1) / run; }
__device__ __host__ inline int mutual_units(int nb, int run) { return nb * mutual_runs(nb, run) + nb; }
__device__ __host__ inline Unit mutual_unit(int nb, int run, int u) {
  const int off = nb * mutual_runs(nb, run);
  if (u >= off) return {u - off, 0, 1};
  const int a = u % nb, d0 = 1 + (u / nb) * run;
  const int last = (nb + 1) / 2 - 1 + ((nb % 2 == 0 && a < nb / 2) ? 1 : 0);
  const int left = last - d0 + 1;
  return {a, d0, left < 0 ? 0 : (left < run ? left : run)};
}

}  // namespace nbm

// ---- mutual.hip: the launch (hipError_t as int, 0 = launched) ----
namespace nbl {
int launch_mutual_pairs_kernel(hipStream_t stream, const nbm::MutualArgs& a);
}  // namespace nbl
