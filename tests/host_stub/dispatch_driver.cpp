// dispatch_driver.cpp — TEST INFRASTRUCTURE (tests/test_force_dispatch.py): calls nbl::launch_force_kernel of the host half of kernels.hip
// over the whole product of what selects a kernel, out-of-range members included (they pin the fallbacks), against dispatch_stub.cpp.
// stdout: one line per case, "<the twelve inputs> -> <what the stub saw>".  `dispatch_driver names` lists the registered kernels instead.
#include <stdio.h>
#include <string.h>

#include "../../mini_nbody_amd/csrc/nbody_internal.hpp"

extern "C" void dispatch_stub_list(FILE* f);

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "names")) { dispatch_stub_list(stdout); return 0; }
  const int variants[] = {0, 1, 2, 3, 4}, Rs[] = {1, 2, 3, 4, 8}, ariths[] = {0, 1, 2, 3, 7}, tiles[] = {0, 256, 512, 1024};
  const int phases[] = {-1, 0, 1, 2, 20, 99}, wsplits[] = {1, 2, 4, 16};
  const size_t ldss[] = {0, 70 * 1024};
  long cases = 0;
  for (int fp64 = 0; fp64 < 2; ++fp64)
  for (int variant : variants)
  for (int R : Rs)
  for (int arith : ariths)
  for (int tile : tiles)
  for (int phase : phases)
  for (int fpga_lds = 0; fpga_lds < 2; ++fpga_lds)
  for (int rows16 = 0; rows16 < 2; ++rows16)
  for (int wsplit : wsplits)
  for (int fpga16 = 0; fpga16 < 2; ++fpga16)
  for (int longb = 0; longb < 2; ++longb)
  for (size_t lds : ldss) {
    nbl::KernelSel s = {fp64, variant, R, arith, tile, phase, fpga_lds, rows16, lds};
    nbk::ForceArgs a;
    memset(&a, 0, sizeof(a));
    a.wsplit = wsplit; a.fpga16 = fpga16; a.long_buffers = longb;
    printf("f%d v%d R%d a%d t%d p%d l%d r%d w%d g%d b%d d%zu -> ", fp64, variant, R, arith, tile, phase, fpga_lds, rows16, wsplit, fpga16, longb, lds);
    const int e = nbl::launch_force_kernel(s, nullptr, dim3(3, 2), a);
    if (e != 0) { printf("error %d\n", e); return 1; }
    ++cases;
  }
  fprintf(stderr, "%ld cases\n", cases);
  return 0;
}
