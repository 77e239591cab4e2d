// device.hip — what hipcc compiles for the library's device code: the force path's translation unit (kernels.hip, unchanged), the
// energy pass's (energy.hip), the field, tidal, jerk and snap passes' (point_sums.hip), the neighbour pass's (neighbors.hip), the k-nearest-neighbour pass's (knn.hip), the friends-of-friends pass's (fof.hip), the radial-count pass's (hist.hip), the pair time-scale pass's (timescale.hip), the pair binding-energy pass's (pair_energy.hip), the Hermite step's elementwise kernels (hermite.hip), the block step's scheduler kernels (hermite_block.hip), the sixth-order Hermite step's elementwise kernels (hermite6.hip), the sixth-order block step's scheduler kernels (hermite6_block.hip) and the mutual pairing's kernel (mutual.hip) as ONE gfx950 code object.  One object, not several: tests/test_strict_rsqrt.py
// reads the strict kernels' branches out of the library's single code object, and a second offload bundle would be a second one.  Each
// file still compiles on its own.  The eight diagnostic passes share diag_pass.hpp (the potential's pair arithmetic, the lane and wave
// preamble, the block and workgroup sizes); with the force path they share nothing beyond reading nbody_args.hpp, and the force
// kernels' machine code is the same either way.
#include "kernels.hip"
#include "energy.hip"
#include "point_sums.hip"
#include "neighbors.hip"
#include "knn.hip"
#include "fof.hip"
#include "hist.hip"
#include "timescale.hip"
#include "pair_energy.hip"
#include "hermite.hip"
#include "hermite_block.hip"
#include "hermite6.hip"
#include "hermite6_block.hip"
#include "mutual.hip"
