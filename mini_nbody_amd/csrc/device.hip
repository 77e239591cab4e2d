// device.hip — what hipcc compiles for the library's device code: the force path's translation unit (kernels.hip, unchanged) and the
// energy pass's (energy.hip) as ONE gfx950 code object.  One object, not two: tests/test_strict_rsqrt.py reads the strict kernels'
// branches out of the library's single code object, and a second offload bundle would be a second one.  Each file still compiles on its
// own and shares nothing with the other beyond nbody_args.hpp; the force kernels' machine code is the same either way.
#include "kernels.hip"
#include "energy.hip"
