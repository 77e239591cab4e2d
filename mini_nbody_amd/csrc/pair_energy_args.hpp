// pair_energy_args.hpp — what pair_energy.cpp (host) and pair_energy.hip (device) agree on: the argument block of the pair binding-energy
// pass and the launch functions of pair_energy.hip.  Like timescale_args.hpp it stays apart from nbody_args.hpp, the force path's hashed
// kernel source.
//
// The result of a row (include/nbody.h, "pair binding energies and binaries") is a minimum of individually rounded pair values, so no
// order has to be defended: an ascending scan over the sources from (e = +inf, idx = -1) that replaces on strict <.  When the sources
// are split over grid.y chunks of whole nbd::kSrcBlock-source blocks, every workgroup stores its chunk's {e, idx} and
// pair_energy_combine takes the chunks in ascending order by the same rule: the same values for every number of chunks.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbpe {

struct PairEnergyArgs {
  const void* src;      // all N position words (16-B or 32-B {x, y, z, w}), ascending
  const void* vsrc;     // all N velocity words in the same layout: {vx, vy, vz, ignored}
  void* e;              // [m] min over j of fma(0.5, v2, -2 / sqrt(d2 + eps)) in the context precision (+inf: no candidate), or null
  int* idx;             // [m] global index of the j that gives it (-1: none), or null
  void* scratch;        // null (grid.y = 1), else the chunks' results: scratch_e / scratch_idx below, each [chunks][m] with row p of
                        // chunk c at c * m + p, so that a wave's 64 stores of one field are contiguous
  int n_src;            // N
  int m;                // rows of this launch
  int first;            // global index of row 0: row p is source first + p and leaves itself out
  int n_blocks;         // ceil(N / nbd::kSrcBlock)
  int chunk_blocks;     // blocks per chunk: workgroup (x, y) walks blocks [y * chunk_blocks, min((y + 1) * chunk_blocks, n_blocks))
  int chunks;           // grid.y = ceil(n_blocks / chunk_blocks): no empty chunk
  // the rows form only: what nbd::query_of reads of a points form is constant here
  static constexpr const void* points = nullptr;
  static constexpr const int* skip = nullptr;
};

// scratch of a launch of m rows over `chunks` chunks: 8 (fp32) or 12 (fp64) bytes per (row, chunk)
inline size_t pair_energy_scratch_bytes(size_t m, size_t chunks, size_t elem) { return m * chunks * (elem + sizeof(int)); }
__host__ __device__ inline void* scratch_e(const PairEnergyArgs& a) { return a.scratch; }
__host__ __device__ inline int* scratch_idx(const PairEnergyArgs& a, size_t elem) {
  return (int*)((char*)a.scratch + (size_t)a.chunks * (size_t)a.m * elem);
}

// what launch_pair_energy_kernel refuses: a bad split (nbd::bad_source_split), a missing source stream, an unsplit launch without an output
inline bool bad_pair_energy_launch(const PairEnergyArgs& a) {
  return nbd::bad_source_split(a, true) || !a.src || !a.vsrc || (!a.scratch && !a.e && !a.idx);
}
// what launch_pair_energy_combine_kernel refuses: nbd::bad_combine's terms and no output to write
inline bool bad_pair_energy_combine(const PairEnergyArgs& a) { return nbd::bad_combine(a) || (!a.e && !a.idx); }

}  // namespace nbpe

namespace nbl {
// both return a hipError_t as int (0 = launched).  grid = (ceil(m / nbd::kLanes), a.chunks); a.chunks > 1 is followed by
// launch_pair_energy_combine_kernel
int launch_pair_energy_kernel(int fp64, hipStream_t stream, const nbpe::PairEnergyArgs& a);
// every row of the launch from a.scratch: chunks ascending, strict <, then e and idx
int launch_pair_energy_combine_kernel(int fp64, hipStream_t stream, const nbpe::PairEnergyArgs& a);
}  // namespace nbl
