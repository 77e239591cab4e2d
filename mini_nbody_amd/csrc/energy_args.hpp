// energy_args.hpp — what energy.cpp (host) and energy.hip (device) agree on: the argument block of the energy pass and the launch
// functions of energy.hip.  Kept apart from nbody_args.hpp, which is part of the force path's hashed kernel source (bench.py
// kernel_source_sha) and is only read here.
//
// The order of every sum (include/nbody.h, "energy and potential") is fixed by N alone:
//   level 1  sources in blocks of kEnergyBlock consecutive bodies, each block summed from zero in ascending order in the context
//            precision, the self pair skipped (with masses: s = fma(m_j, inv, s), the self pair leaves s as it is);
//   level 2  the block sums converted to fp64 and added in ascending block order from zero: L2_i;  phi_i = 0 - L2_i.
// Totals (one rank's rows): rows in groups of kEnergyRows from the rank's first body, each group summed in ascending row order in
// fp64 (one partial per workgroup), then the groups' partials in ascending order (energy_reduce).  With masses a row's eight terms
// are each one fp64 product more: mi = (double)w_i times the unit-mass term.
#pragma once
#include <hip/hip_runtime.h>

#include "diag_pass.hpp"

namespace nbe {

constexpr int kEnergyBlock = nbd::kSrcBlock;   // sources per level-1 block
constexpr int kEnergyRows = nbd::kLanes;        // rows per workgroup = per partial of the totals
constexpr int kEnergyWords = 8;      // {T, U, Px, Py, Pz, Lx, Ly, Lz} = NBODY_ENERGY_*

struct EnergyArgs {
  const void* src;   // all N source words (16-B or 32-B {x, y, z, w}), ascending
  const void* vel;   // the rank's n_local velocity words (null: no totals)
  void* phi;         // [row_count] phi_i in the context precision, or null
  double* part;      // [ceil(row_count / kEnergyRows)][kEnergyWords] per-workgroup fp64 sums, or null
  int n_src;         // N
  int first;         // global index of the rank's row 0
  int row0;          // first row (of the rank's slice) this launch handles
  int row_count;     // rows handled
  int masses;        // NBODY_OPT_MASSES: 1 = s = fma(m_j, inv, s) with m_j the w of source j's word, and the rows' terms of the totals
                     // times (double)w_i; 0 = unit masses, w is not read
};

}  // namespace nbe

namespace nbl {
// both return a hipError_t as int (0 = launched).  arith: NBODY_ARITH_* (fp64 contexts: strict or not)
int launch_energy_kernel(int fp64, int arith, hipStream_t stream, const nbe::EnergyArgs& a);
// out[q] = sum over g ascending of part[g][q], q = 0..7, with T and U halved (one workgroup)
int launch_energy_reduce_kernel(hipStream_t stream, const double* part, int groups, double* out);
}  // namespace nbl
