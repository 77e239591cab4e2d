// kernels.hip — the one device translation unit of libnbody_hip.so: the kernels of nbody_kernels.hpp and the launch functions that
// pick an instantiation (namespace nbl, declared in nbody_internal.hpp).  No context, no options, no policy here: WHAT to launch is
// decided in context.cpp (launch_force) and arrives as a KernelSel + ForceArgs; this file turns that into one hipLaunchKernelGGL.
// gfx950 only.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "nbody_internal.hpp"
#include "nbody_kernels.hpp"

using namespace nbk;

#define NBL_HIDDEN __attribute__((visibility("hidden")))

namespace {

// Every force kernel has the signature void(ForceArgs): which one a launch takes is a function of KernelSel and of three fields of
// ForceArgs (wsplit, fpga16, long_buffers), written once here.  tests/test_force_dispatch.py pins it, fallbacks included.
using ForceKernel = void (*)(ForceArgs);

template <int... Cs> using Ints = std::integer_sequence<int, Cs...>;
// a run-time value as a compile-time constant: f(std::integral_constant<int, C>) for the first C of the list that equals v, for the
// LAST of the list when none does (the fallback)
template <int C, int... Rest, typename F>
ForceKernel on_value(Ints<C, Rest...>, int v, F f) {
  if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, C>{});
  else return v == C ? f(std::integral_constant<int, C>{}) : on_value(Ints<Rest...>{}, v, f);
}
template <typename F> ForceKernel on_arith(int arith, F f) { return on_value(Ints<NBODY_ARITH_REFERENCE, NBODY_ARITH_STRICT, NBODY_ARITH_REFERENCE_STRICT, 0>{}, arith, f); }
template <typename F> ForceKernel on_wsplit(int wsplit, F f) { return on_value(Ints<16, 4, 1>{}, wsplit, f); }
// bodies per lane: 8 only exists in fp32 (and there only for the SMEM kernel, see below)
template <bool FP64, typename F> ForceKernel on_rows_per_lane(int R, F f) {
  if constexpr (FP64) return on_value(Ints<1, 2, 4>{}, R, f);
  else return on_value(Ints<1, 2, 8, 4>{}, R, f);
}
template <typename F> ForceKernel on_lds_tile(int tile, F f) { return on_value(Ints<1024, 512, 256>{}, tile >= 1024 ? 1024 : tile >= 512 ? 512 : 256, f); }
// the forms of the hand-scheduled loops (NBODY_OPT_ISA_PHASE); whatever is not in a list runs the product loop, form 1
using IsaPhasesF64 = Ints<2, 0, 1>;
#ifdef NBODY_DIAG_LOOPS   // the diagnostic build only extends the list (NB_DIAG_LOOP_FORMS, nbody_kernels.hpp: some are TIMING-ONLY, WRONG RESULTS)
#define NB_LIST_FORM(N) N,
using IsaPhasesF32 = Ints<0, NB_DIAG_LOOP_FORMS(NB_LIST_FORM) 1>;
#undef NB_LIST_FORM
#else
using IsaPhasesF32 = Ints<0, 1>;
#endif

// the 16-row FPGA kernel: small launches of ONE segment, sixteen rows x sixteen chains per 256-thread workgroup (grid.x counts 16-row units)
bool takes_fpga_rows16(const nbl::KernelSel& s, const ForceArgs& a) { return !s.fp64 && a.fpga16 && s.fpga_rows16; }

ForceKernel select_force_kernel(const nbl::KernelSel& s, const ForceArgs& a) {
  if (s.fp64 && s.variant == NBODY_VARIANT_ISA)
    return on_value(IsaPhasesF64{}, s.isa_phase, [&](auto PH) {
      return on_wsplit(a.wsplit, [](auto WS) -> ForceKernel { return force_isa_f64<decltype(PH)::value, decltype(WS)::value>; });
    });
  if (s.fp64)   // STRICT = NBODY_ARITH_STRICT / _REFERENCE_STRICT: IEEE 1/sqrt (fp64 has one d2 form: the bit-0 distinction is fp32's)
    return on_value(Ints<1, 0>{}, (s.arith & 2) ? 1 : 0, [&](auto STRICT) {
      return on_rows_per_lane<true>(s.R, [&](auto R) -> ForceKernel {
        constexpr int r = decltype(R)::value, strict = decltype(STRICT)::value;
        if constexpr (r == 1) return on_wsplit(a.wsplit, [](auto WS) -> ForceKernel { return force_smem_f64<1, decltype(WS)::value, strict>; });
        else return force_smem_f64<r, 1, strict>;   // the wave split is for one body per lane
      });
    });
  if (a.fpga16)
    return on_arith(s.arith, [&](auto A) -> ForceKernel {
      constexpr int arith = decltype(A)::value;
      if (s.fpga_rows16) return force_fpga16r_f32<arith>;
      if (a.wsplit != 16) return force_fpga16_f32<arith>;
      return s.fpga_lds ? force_fpga16w_lds_f32<arith>     // sources staged through LDS (the default of the sixteen-wave form)
                        : force_fpga16w_f32<arith>;
    });
  if (s.variant == NBODY_VARIANT_ISA) {   // one body per lane, fast arithmetic only (resolve_config guarantees both)
    if (a.long_buffers) return on_wsplit(a.wsplit, [](auto WS) -> ForceKernel { return force_isa_long_f32<decltype(WS)::value>; });
    return on_value(IsaPhasesF32{}, s.isa_phase, [&](auto PH) {
      return on_wsplit(a.wsplit, [](auto WS) -> ForceKernel {
        // the 16-wave form exists for the product loop and its placement twin (resolve_config sees to it)
        constexpr int ph = decltype(PH)::value, ws = (ph <= 1 || decltype(WS)::value != 16) ? decltype(WS)::value : 1;
        return force_isa_f32<ph, ws>;
      });
    });
  }
  return on_rows_per_lane<false>(s.R, [&](auto R) {
    return on_arith(s.arith, [&](auto A) -> ForceKernel {
      constexpr int r = decltype(R)::value, arith = decltype(A)::value;
      if constexpr (r != 8) {   // 8 bodies per lane only exists for the SMEM variant
        if (s.variant == NBODY_VARIANT_LDS) return on_lds_tile(s.tile, [](auto TILE) -> ForceKernel { return force_lds_f32<r, arith, decltype(TILE)::value>; });
        if (s.variant == NBODY_VARIANT_READLANE) return force_readlane_f32<r, arith>;
      }
      if constexpr (r == 1) return on_wsplit(a.wsplit, [](auto WS) -> ForceKernel { return force_smem_f32<1, arith, decltype(WS)::value>; });
      else return force_smem_f32<r, arith, 1>;
    });
  });
}

}  // namespace

namespace nbl {

NBL_HIDDEN bool diag_build() {
#ifdef NBODY_DIAG_LOOPS
  return true;
#else
  return false;
#endif
}

NBL_HIDDEN int launch_force_kernel(const KernelSel& s, hipStream_t st, dim3 grid, const ForceArgs& a) {
  const ForceKernel kernel = select_force_kernel(s, a);
  const bool rows16 = takes_fpga_rows16(s, a);   // its own block shape; launched without dynamic LDS, hence without the attribute call
  const size_t dyn_lds = rows16 ? 0 : s.dyn_lds;
  if (dyn_lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(rows16 ? 256 : wg_threads(a.wsplit)), dyn_lds, st, a);
  return (int)hipGetLastError();
}

// the two-launch form (NBODY_OPT_FUSE_COMBINE = 0): after the step's last force launch, add the partials
NBL_HIDDEN int launch_combine_kernel(int fp64, hipStream_t st, dim3 grid, const ForceArgs& c) {
  if (fp64) hipLaunchKernelGGL((combine_kernel<double, d4>), grid, dim3(kBlock), 0, st, c);
  else hipLaunchKernelGGL((combine_kernel<float, f4>), grid, dim3(kBlock), 0, st, c);
  return (int)hipGetLastError();
}

NBL_HIDDEN int launch_drift_kernel(int fp64, hipStream_t st, void* pos_rows, const void* vel, int n_rows, float dt, double dt64) {
  if (n_rows <= 0) return 0;
  dim3 grid((n_rows + kBlock - 1) / kBlock);
  if (fp64) hipLaunchKernelGGL((drift_kernel<double, d4>), grid, dim3(kBlock), 0, st, (d4*)pos_rows, (const d4*)vel, n_rows, dt, dt64);
  else hipLaunchKernelGGL((drift_kernel<float, f4>), grid, dim3(kBlock), 0, st, (f4*)pos_rows, (const f4*)vel, n_rows, dt, dt64);
  return (int)hipGetLastError();
}

// RAM A's read port: body words of the host's RAM image into the resident source array (S/top_level.vhd:206-208, 238-240); t0 (may be
// null): where its first wave stamps the start of the request's tick count
NBL_HIDDEN int launch_ingest_kernel(hipStream_t st, void* dst_words, const void* ram_a_bodies, int n, unsigned long long* t0) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(ingest_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (f4*)dst_words, (const f4*)ram_a_bodies, n, t0);
  return (int)hipGetLastError();
}

// `complete` written by the device: word 0 of RAM A <- {ticks, BEGIN = 0}, then the library's sequence word (S/top_level.vhd:255-263)
NBL_HIDDEN int launch_mailbox_done_kernel(hipStream_t st, void* word0, unsigned* seq_word, const unsigned long long* t0, unsigned seq,
                                          unsigned clock_khz, unsigned rt_khz) {
  hipLaunchKernelGGL(mailbox_done_kernel, dim3(1), dim3(64), 0, st, (unsigned*)word0, seq_word, t0, seq, clock_khz, rt_khz);
  return (int)hipGetLastError();
}

NBL_HIDDEN int launch_rsqrt_selftest_kernel(unsigned first_bits, unsigned long long count, unsigned long long* out3) {
  const unsigned long long wgs = (count + 255) / 256;
  rsqrt_selftest_kernel<<<dim3((unsigned)(wgs < 16384 ? wgs : 16384)), dim3(256)>>>(first_bits, count, out3);
  return (int)hipGetLastError();
}

NBL_HIDDEN int launch_rsqrt_array_kernel(const float* x, float* y, int n, int ieee_only) {
  rsqrt_array_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(x, y, n, ieee_only ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace nbl
