// hermite_host.hpp — what hermite.cpp shares with hermite_block.cpp (host C++ only): the opening of a Hermite call, the gathers that
// bring the predicted state of all bodies to every device and rank, and the mark of a rewritten own slice.  hermite.cpp defines them;
// none refers to a device symbol beyond those of hermite.hip and point_sums.hip.
#pragma once
#include "query_pass.hpp"

namespace nbi {

// what every Hermite call starts with: the configuration, the buffers of a call (he_*), (a0, j0) of the state it finds into he_*[0]
int hermite_open_call();
// The live buffers' own slices have been rewritten (a predictor): positions and velocities of ALL bodies to every device and rank,
// with the drains an evaluation needs before and after (hermite.cpp says why); what follows is a jerk pass on every local
int hermite_gather_state();
// the own slice of pos[cur] has been rewritten on L's compute stream: what the next gather waits for
int hermite_own_slice_written(Local& L);

}  // namespace nbi
