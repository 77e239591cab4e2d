# Top-level build: the HIP library (the product), the C host program, the oracle (test infrastructure)
# and the microbenchmark.  gfx950 only.  `python -c "import __graft_entry__ as g; g.build()"` runs this.
HIPCC   ?= hipcc
CC      ?= gcc
ARCH    ?= gfx950
PKG     := mini_nbody_amd
CSRC    := $(PKG)/csrc
# -ffp-contract=off: products are fused only where the source says fma (rounding points are part of the contract)
# -fno-slp-vectorize: v_pk_*_f32 costs 4 cycles on gfx950 (profiles/r01_microbench_valu_issue.txt): no gain, more registers
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-function

all: lib host oracle microbench

# The library = ONE device code object (device.hip: the force path's kernels.hip — the nbk kernels + the launch functions that pick an
# instantiation, ~45 s of hipcc — the energy pass's energy.hip, the field, tidal, jerk and snap passes' point_sums.hip, the neighbour pass's neighbors.hip, the k-nearest-neighbour pass's knn.hip, the friends-of-friends pass's fof.hip, the radial-count pass's hist.hip, the pair time-scale pass's timescale.hip, the pair binding-energy pass's pair_energy.hip, the Hermite step's hermite.hip, the block step's hermite_block.hip, the sixth-order Hermite step's hermite6.hip and the sixth-order block step's hermite6_block.hip) and fifteen
# host-only C++ files (context, comm, mailbox, energy, point_sums, neighbors, knn, fof, hist, timescale, pair_energy, hermite, hermite_block, hermite6, hermite6_block: seconds each) behind csrc/nbody_internal.hpp.  A host-side edit relinks in seconds.
# The eight diagnostic passes share csrc/diag_pass.hpp (device code — the distance passes' pair distance and query preamble included — the sizes
# their hosts read and the guard of a split launch) and csrc/query_pass.hpp (host only: the flow of a call and the two split rules).
HOSTFLAGS := -O2 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function
OBJ      := build/obj
KERNEL_SRC := $(CSRC)/kernels.hip $(CSRC)/nbody_kernels.hpp $(CSRC)/nbody_args.hpp $(CSRC)/force_loop_gfx950.inc
HOST_HDR := $(CSRC)/nbody_internal.hpp $(CSRC)/nbody_args.hpp $(CSRC)/query_pass.hpp $(CSRC)/diag_pass.hpp include/nbody.h
HOST_OBJ := $(OBJ)/context.o $(OBJ)/comm.o $(OBJ)/mailbox.o $(OBJ)/energy.o $(OBJ)/point_sums.o $(OBJ)/neighbors.o $(OBJ)/knn.o $(OBJ)/fof.o $(OBJ)/hist.o $(OBJ)/timescale.o $(OBJ)/pair_energy.o $(OBJ)/hermite.o $(OBJ)/hermite_block.o $(OBJ)/hermite6.o $(OBJ)/hermite6_block.o $(OBJ)/mutual.o
# the energy diagnostics' device code (energy.hip, seconds of hipcc on its own) reads nbody_args.hpp and changes nothing of the force path's
# hashed source (KERNEL_SRC); device.hip compiles it with kernels.hip into the library's one code object.  Its host side is energy.cpp, one
# of HOST_OBJ.  What it shares with the seven passes below is diag_pass.hpp, which is no part of the hashed source either.
ENERGY_SRC := $(CSRC)/energy.hip $(CSRC)/energy_args.hpp
# the field pass (acceleration and potential at arbitrary points), the tidal pass (the tidal tensor there, the gradient of the field) and
# the jerk pass (the field's time derivative at rows and phase-space points) and the snap pass (its second time derivative) in the same way, the four as one: point_sums.hip beside
# energy.hip, point_sums.cpp one of HOST_OBJ
POINT_SUMS_SRC := $(CSRC)/point_sums.hip $(CSRC)/point_sums_args.hpp
# the neighbour pass (nearest body, radius count, closest pair) likewise: neighbors.hip beside point_sums.hip, neighbors.cpp one of HOST_OBJ
NEIGHBORS_SRC := $(CSRC)/neighbors.hip $(CSRC)/neighbors_args.hpp
# the k-nearest-neighbour pass (the k nearest bodies and their distances) likewise: knn.hip beside neighbors.hip, knn.cpp one of HOST_OBJ
KNN_SRC := $(CSRC)/knn.hip $(CSRC)/knn_args.hpp
# the friends-of-friends pass (the groups of a linking length) likewise: fof.hip beside knn.hip, fof.cpp one of HOST_OBJ
FOF_SRC := $(CSRC)/fof.hip $(CSRC)/fof_args.hpp
# the radial-count pass (bodies per shell of distance, the pair histogram) likewise: hist.hip beside fof.hip, hist.cpp one of HOST_OBJ
HIST_SRC := $(CSRC)/hist.hip $(CSRC)/hist_args.hpp
# the pair time-scale pass (pair crossing times, the closest distance, the shared adaptive step) likewise: timescale.hip beside hist.hip, timescale.cpp one of HOST_OBJ
TIMESCALE_SRC := $(CSRC)/timescale.hip $(CSRC)/timescale_args.hpp
# the pair binding-energy pass (every body's most bound partner, the binaries and their elements) likewise: pair_energy.hip beside timescale.hip, with
# which it shares diag_pass.hpp's pair_walk; pair_energy.cpp one of HOST_OBJ
PAIR_ENERGY_SRC := $(CSRC)/pair_energy.hip $(CSRC)/pair_energy_args.hpp
# the Hermite step's elementwise kernels (predictor, corrector, the best-row reduction) likewise: hermite.hip beside timescale.hip, hermite.cpp one
# of HOST_OBJ; its all-pairs work is the jerk pass of point_sums.hip
HERMITE_SRC := $(CSRC)/hermite.hip $(CSRC)/hermite_args.hpp
# the block step's scheduler kernels (individual block time steps: init, predict-to-tau, next-time, compact-and-gather, correct-and-assign)
# likewise: hermite_block.hip beside hermite.hip, hermite_block.cpp one of HOST_OBJ; it shares hermite.cpp's opening and gathers through
# hermite_host.hpp, and its all-pairs work is the jerk points pass of point_sums.hip
HERMITE_BLOCK_SRC := $(CSRC)/hermite_block.hip $(CSRC)/hermite_block_args.hpp
# the sixth-order Hermite step's elementwise kernels (predictor, corrector with the crackle) likewise: hermite6.hip beside hermite_block.hip,
# hermite6.cpp one of HOST_OBJ; it shares hermite.cpp's buffers, gathers, minimum and adaptive loop through hermite_host.hpp, and its
# all-pairs work is the snap pass of point_sums.hip
HERMITE6_SRC := $(CSRC)/hermite6.hip $(CSRC)/hermite6_args.hpp
# the sixth-order block step's scheduler kernels (init, predict-to-tau, compact-and-gather, correct-and-assign) likewise: hermite6_block.hip
# beside hermite6.hip, hermite6_block.cpp one of HOST_OBJ; it opens as hermite6.cpp does and reads the next time as hermite_block.cpp does
# (hermite_host.hpp), and its all-pairs work is the snap points pass of point_sums.hip
HERMITE6_BLOCK_SRC := $(CSRC)/hermite6_block.hip $(CSRC)/hermite6_block_args.hpp
# the mutual pairing of the full fp32 force pass (every unordered pair once, the ordered pass's bits): mutual.hip beside hermite6.hip — it reads
# nbody_kernels.hpp for apply_force and changes nothing of it — mutual.cpp one of HOST_OBJ.  Its unit loop is generated
# (tools/gen_mutual_loop.py -> mutual_loop_gfx950.inc, committed): `make lib` rebuilds the code object when it changes
MUTUAL_SRC := $(CSRC)/mutual.hip $(CSRC)/mutual_args.hpp $(CSRC)/mutual_loop_gfx950.inc
DEVICE_SRC := $(CSRC)/device.hip $(KERNEL_SRC) $(CSRC)/diag_pass.hpp $(ENERGY_SRC) $(POINT_SUMS_SRC) $(NEIGHBORS_SRC) $(KNN_SRC) $(FOF_SRC) $(HIST_SRC) $(TIMESCALE_SRC) $(PAIR_ENERGY_SRC) $(HERMITE_SRC) $(HERMITE_BLOCK_SRC) $(HERMITE6_SRC) $(HERMITE6_BLOCK_SRC) $(MUTUAL_SRC)

lib: $(PKG)/libnbody_hip.so
$(OBJ)/device.o: $(DEVICE_SRC) $(HOST_HDR)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/device.hip -o $@
$(OBJ)/%.o: $(CSRC)/%.cpp $(HOST_HDR)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@
$(OBJ)/energy.o: $(CSRC)/energy_args.hpp
$(OBJ)/point_sums.o: $(CSRC)/point_sums_args.hpp
$(OBJ)/neighbors.o: $(CSRC)/neighbors_args.hpp
$(OBJ)/knn.o: $(CSRC)/knn_args.hpp
$(OBJ)/fof.o: $(CSRC)/fof_args.hpp
$(OBJ)/hist.o: $(CSRC)/hist_args.hpp
$(OBJ)/timescale.o: $(CSRC)/timescale_args.hpp
$(OBJ)/pair_energy.o: $(CSRC)/pair_energy_args.hpp
$(OBJ)/hermite.o: $(CSRC)/hermite_args.hpp $(CSRC)/hermite_host.hpp
$(OBJ)/hermite_block.o: $(CSRC)/hermite_args.hpp $(CSRC)/hermite_host.hpp $(CSRC)/hermite_block_args.hpp
$(OBJ)/hermite6.o: $(CSRC)/hermite6_args.hpp $(CSRC)/hermite_host.hpp
$(OBJ)/hermite6_block.o: $(CSRC)/hermite_args.hpp $(CSRC)/hermite_host.hpp $(CSRC)/hermite_block_args.hpp $(CSRC)/hermite6_args.hpp $(CSRC)/hermite6_block_args.hpp
$(OBJ)/mutual.o: $(CSRC)/mutual_args.hpp
$(PKG)/libnbody_hip.so: $(OBJ)/device.o $(HOST_OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -pthread -o $@ $^ -ldl

# The diagnostic library: the same sources with kernels.hip built -DNBODY_DIAG_LOOPS — the experiment encodings of the hand-scheduled loop
# and its TIMING-ONLY forms (wrong results) that profiles/r02_loop_diagnostics.md was measured with.  Not part of `all`, never loaded by
# the package unless NBODY_LIB points at it (tools/profile_diag.sh does).  The host objects are the product's own.
diag: $(PKG)/libnbody_hip_diag.so
$(OBJ)/device_diag.o: $(DEVICE_SRC) $(HOST_HDR)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DNBODY_DIAG_LOOPS -c $(CSRC)/device.hip -o $@
$(PKG)/libnbody_hip_diag.so: $(OBJ)/device_diag.o $(HOST_OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -pthread -o $@ $^ -ldl

# C host program (north_star: "host code stays in C"): links only the C-ABI
host: build/nbody build/mailbox_driver
build/nbody: $(PKG)/host/nbody.c include/nbody.h include/nbody_ic.h $(PKG)/libnbody_hip.so
	@mkdir -p build
	$(CC) -std=c11 -O2 -Wall -Iinclude -o $@ $(PKG)/host/nbody.c -L$(PKG) -lnbody_hip -Wl,-rpath,'$$ORIGIN/../$(PKG)' -Wl,-rpath,/opt/rocm/lib -lm

# the PS-side driver of the reference's mailbox, plain C over the same C-ABI
build/mailbox_driver: $(PKG)/host/mailbox_driver.c include/nbody.h include/nbody_ic.h $(PKG)/libnbody_hip.so
	@mkdir -p build
	$(CC) -std=c11 -O2 -Wall -Iinclude -o $@ $(PKG)/host/mailbox_driver.c -L$(PKG) -lnbody_hip -Wl,-rpath,'$$ORIGIN/../$(PKG)' -Wl,-rpath,/opt/rocm/lib -lm

oracle:
	$(MAKE) -C oracle

microbench: build/microbench build/microbench_streams build/microbench_roles build/microbench_mfma build/microbench_gridsync
build/microbench: $(CSRC)/microbench.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
build/microbench_roles: $(CSRC)/microbench_roles.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
# 0.5 MB of generated instruction streams: produced on demand, not tracked
$(CSRC)/microbench_streams.inc: tools/gen_streams.py tools/gen_force_loop.py tools/gen_mutual_loop.py
	python3 tools/gen_streams.py
build/microbench_streams: $(CSRC)/microbench_streams.hip $(CSRC)/microbench_streams.inc
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<

# round 4's probe: can the matrix pipe carry the coordinate differences? (no: profiles/r04_mfma_differences.md); its loop is generated
$(CSRC)/force_loop_mfma_gfx950.inc: tools/gen_mfma_loop.py
	python3 tools/gen_mfma_loop.py
build/microbench_mfma: $(CSRC)/microbench_mfma.hip $(CSRC)/force_loop_mfma_gfx950.inc
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -ffp-contract=off -fno-slp-vectorize -o $@ $<

# round 4: what a step boundary costs inside a launch against the kernel boundary (profiles/r04_step_boundary.md)
build/microbench_gridsync: $(CSRC)/microbench_gridsync.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<

# generated sources: the hand-scheduled loops (committed) and the microbenchmark streams (not tracked)
gen:
	python3 tools/gen_force_loop.py
	python3 tools/gen_mutual_loop.py
	python3 tools/gen_streams.py

isa: $(KERNEL_SRC)
	@mkdir -p build/isa
	cd build/isa && $(HIPCC) $(HIPFLAGS) -c ../../$(CSRC)/kernels.hip -save-temps -Rpass-analysis=kernel-resource-usage -o kernels.o 2> resource_usage.txt

clean:
	rm -rf build $(PKG)/libnbody_hip.so $(PKG)/libnbody_hip_diag.so
	$(MAKE) -C oracle clean

.PHONY: all lib diag host oracle microbench isa gen clean
