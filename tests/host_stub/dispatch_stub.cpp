// dispatch_stub.cpp — TEST INFRASTRUCTURE (tests/test_force_dispatch.py): the eight entry points of the HIP runtime that the HOST half of
// kernels.hip (compiled --cuda-host-only) needs, so that which kernel a launch takes can be read on a machine without a GPU.  At
// registration it records host pointer -> device name; a launch prints the device name, the block size, the dynamic LDS and the value of
// the dynamic-LDS attribute if hipFuncSetAttribute was called for that kernel since the last launch (0: it was not).  Nothing runs.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <map>
#include <string>

namespace {
std::map<const void*, std::string>& names() { static std::map<const void*, std::string> m; return m; }   // (used from static constructors)
struct Config { dim3 grid, block; size_t lds; hipStream_t stream; } g_cfg;
const void* g_attr_fn = nullptr;
int g_attr_value = 0;
const char* name_of(const void* fn) { auto it = names().find(fn); return it == names().end() ? "UNREGISTERED" : it->second.c_str(); }
}  // namespace

// every registered device name, one per line (the "same instantiations exist" check)
extern "C" void dispatch_stub_list(FILE* f) { for (auto& kv : names()) fprintf(f, "%s\n", kv.second.c_str()); }

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
  names()[host_fn] = device_name;
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) { g_cfg = {grid, block, lds, stream}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
  *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *stream = g_cfg.stream;
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute attr, int value) {
  if (attr != hipFuncAttributeMaxDynamicSharedMemorySize) return hipErrorInvalidValue;
  g_attr_fn = fn; g_attr_value = value;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void**, size_t lds, hipStream_t) {
  const bool other = g_attr_fn && g_attr_fn != fn;   // the attribute went to a kernel that is not the one launched
  printf("%s block=%u lds=%zu attr=%d%s%s\n", name_of(fn), block.x, lds, g_attr_fn == fn ? g_attr_value : 0, other ? " attr-on=" : "",
         other ? name_of(g_attr_fn) : "");
  g_attr_fn = nullptr; g_attr_value = 0;
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}
