// masses_stub.cpp — TEST INFRASTRUCTURE (tests/test_masses_host_sanitizers.py): hip_stub.cpp as it is, and stand-ins for the launch
// functions of energy.hip and point_sums.hip that echo the `masses` member of the REAL EnergyArgs and PointSumsArgs, so that a driver on
// a machine without a GPU can see NBODY_OPT_MASSES arrive in both argument blocks under AddressSanitizer / UBSan.
//   energy      hip_stub.cpp's stand-in (its values unchanged), after the flag of the launch has been noted: masses_stub_energy_flag()
//               returns the flag of the last launch, masses_stub_energy_launches() how many there were
//   point sums  every value of every output asked for, of all m queries: (T)(1 + masses) from an unsplit launch, (T)(3 + masses) from the
//               combine of a split one (whose first launch writes the flag into every scratch word it owns, and the combine checks them);
//               refused by the real predicates of point_sums_args.hpp
// It says nothing about the kernels' arithmetic (the GPU tests do).  Linked INSTEAD of hip_stub.cpp, which it includes.
#define launch_energy_kernel launch_energy_kernel_unflagged
#include "hip_stub.cpp"
#undef launch_energy_kernel

#include "../../mini_nbody_amd/csrc/point_sums_args.hpp"

namespace {

int g_energy_flag = -1;
long g_energy_launches = 0;

template <typename T>
void fill_outputs(const nbp::PointPass& pass, const nbp::PointSumsArgs& a, T value) {
  for (int i = 0; i < 2; ++i)
    if (a.out[i])
      for (size_t k = 0; k < (size_t)a.m * (size_t)pass.out_values[i]; ++k) ((T*)a.out[i])[k] = value;
}

template <typename T>
int sums(const nbp::PointPass& pass, const nbp::PointSumsArgs& a) {
  if (!a.scratch) { fill_outputs<T>(pass, a, (T)(1 + a.masses)); return 0; }
  const size_t words = nbp::point_sums_scratch_bytes((size_t)a.m, (size_t)a.n_blocks, (size_t)pass.sums, sizeof(T)) / sizeof(T);
  for (size_t k = 0; k < words; ++k) ((T*)a.scratch)[k] = (T)a.masses;
  return 0;
}

template <typename T>
int combine(const nbp::PointPass& pass, const nbp::PointSumsArgs& a) {
  const size_t words = nbp::point_sums_scratch_bytes((size_t)a.m, (size_t)a.n_blocks, (size_t)pass.sums, sizeof(T)) / sizeof(T);
  for (size_t k = 0; k < words; ++k)
    if (((const T*)a.scratch)[k] != (T)a.masses) return (int)hipErrorInvalidValue;   // the two launches of a split saw one flag
  fill_outputs<T>(pass, a, (T)(3 + a.masses));
  return 0;
}

}  // namespace

extern "C" int masses_stub_energy_flag(void) { return g_energy_flag; }
extern "C" long masses_stub_energy_launches(void) { return g_energy_launches; }

namespace nbl {
int launch_energy_kernel_unflagged(int fp64, int arith, hipStream_t stream, const nbe::EnergyArgs& a);
int launch_energy_kernel(int fp64, int arith, hipStream_t stream, const nbe::EnergyArgs& a) {
  g_energy_flag = a.masses;
  ++g_energy_launches;
  return launch_energy_kernel_unflagged(fp64, arith, stream, a);
}
int launch_point_sums_kernel(const nbp::PointPass& pass, int fp64, int, hipStream_t, int chunks, const nbp::PointSumsArgs& a) {
  if (nbp::bad_point_sums_launch(a, chunks) || nbp::bad_point_sums_queries(pass, a)) return (int)hipErrorInvalidValue;
  if (a.masses != 0 && a.masses != 1) return (int)hipErrorInvalidValue;
  return fp64 ? sums<double>(pass, a) : sums<float>(pass, a);
}
int launch_point_sums_combine_kernel(const nbp::PointPass& pass, int fp64, hipStream_t, const nbp::PointSumsArgs& a) {
  if (nbp::bad_point_sums_combine(a)) return (int)hipErrorInvalidValue;
  return fp64 ? combine<double>(pass, a) : combine<float>(pass, a);
}
}  // namespace nbl
