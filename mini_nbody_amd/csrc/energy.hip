// energy.hip — the energy pass's device code: the all-pairs potential phi_i of every row and the per-workgroup fp64 partial sums of
// {T, U, P, L}, then one small launch that adds the partials (energy_args.hpp states the order, include/nbody.h the definitions).
// Compiles on its own; device.hip puts it into the library's one code object next to kernels.hip.  Reads nbody_args.hpp (f4, d4)
// and nothing else of the force path; the pair arithmetic of the potential is diag_pass.hpp's inv_dist.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "energy_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbe;
using namespace nbd;

#define NBE_HIDDEN __attribute__((visibility("hidden")))

namespace {

// One row per lane, kEnergyRows rows per workgroup, every lane walks all N sources in kEnergyBlock blocks.  Sources arrive with
// wave-uniform scalar loads (address space 4, as force_smem_f32).  The self pair is skipped by a wave-uniform branch: only the one or two
// aligned 64-source windows that overlap the wave's own 64 rows compare j with i (adding 0 in place of the self term changes no bit of a
// sum of non-negative terms); every other window is 3 sub, 3 fma, 1 rsq and 1 add per pair.
// MASS (EnergyArgs::masses): s = fma(m_j, inv, s) with m_j the w of the source's word, and the self pair is a select on s — with
// masses of either sign or a NaN the sum's terms are not non-negative, so the row's own term must not enter at all.  The rows' terms
// of the totals are then mi = (double)w_i times the unit-mass terms, one fp64 product each.  MASS = false is the code it was.
template <bool MASS, typename T>
__device__ __forceinline__ T add_pair(T m, T inv, T s, bool self) {
  if constexpr (MASS) return self ? s : fma_of(m, inv, s);
  else return s + (self ? (T)0 : inv);
}

template <typename T, typename V4, int ARITH, bool MASS>
__global__ void __launch_bounds__(kEnergyRows) energy_kernel(EnergyArgs a) {
  __shared__ double red[kEnergyWords][kEnergyRows];
  const int row_end = a.row0 + a.row_count;
  const int base = a.row0 + (int)blockIdx.x * kEnergyRows;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lr = base + (int)threadIdx.x;
  const bool live = lr < row_end;
  const int i = a.first + (live ? lr : row_end - 1);
  const int wlo = a.first + min(base + wave * 64, row_end - 1);        // the wave's rows, global, inclusive
  const int whi = a.first + min(base + wave * 64 + 63, row_end - 1);
  const V4 me = ((const V4*)a.src)[i];
  const T eps = soft<T>();
  const NB_CONST V4* src = (const NB_CONST V4*)(uintptr_t)a.src;
  double l2 = 0.0;
  for (int b0 = 0; b0 < a.n_src; b0 += kEnergyBlock) {
    const int b1 = min(b0 + kEnergyBlock, a.n_src);
    T s = 0;
    int j = b0;
    for (; j + 64 <= b1; j += 64) {
      if (j + 63 < wlo || j > whi) {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) {
          const V4 p = src[j + k];
          const T t = inv_dist<ARITH>(p.x - me.x, p.y - me.y, p.z - me.z, eps);
          if constexpr (MASS) s = fma_of(p.w, t, s);
          else s += t;
        }
      } else {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) {
          const V4 p = src[j + k];
          const T t = inv_dist<ARITH>(p.x - me.x, p.y - me.y, p.z - me.z, eps);
          s = add_pair<MASS>(p.w, t, s, j + k == i);
        }
      }
    }
    for (; j < b1; ++j) {   // the last block's tail (N not a multiple of 64)
      const V4 p = src[j];
      const T t = inv_dist<ARITH>(p.x - me.x, p.y - me.y, p.z - me.z, eps);
      s = add_pair<MASS>(p.w, t, s, j == i);
    }
    l2 += (double)s;
  }
  const double u = 0.0 - l2;                       // phi_i (N = 1: +0)
  if (a.phi && live) ((T*)a.phi)[lr - a.row0] = (T)u;
  if (!a.part) return;
  const V4 v = ((const V4*)a.vel)[live ? lr : row_end - 1];
  const double x = me.x, y = me.y, z = me.z, vx = v.x, vy = v.y, vz = v.z;
  const int t = (int)threadIdx.x;
  if constexpr (MASS) {
    const double mi = me.w;
    red[0][t] = mi * __builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz));
    red[1][t] = mi * u;
    red[2][t] = mi * vx; red[3][t] = mi * vy; red[4][t] = mi * vz;
    red[5][t] = mi * (y * vz - z * vy);
    red[6][t] = mi * (z * vx - x * vz);
    red[7][t] = mi * (x * vy - y * vx);
  } else {
    red[0][t] = __builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz));
    red[1][t] = u;
    red[2][t] = vx; red[3][t] = vy; red[4][t] = vz;
    red[5][t] = y * vz - z * vy;
    red[6][t] = z * vx - x * vz;
    red[7][t] = x * vy - y * vx;
  }
  __syncthreads();
  if (t < kEnergyWords) {
    const int cnt = min(kEnergyRows, row_end - base);
    double acc = 0.0;
    for (int r = 0; r < cnt; ++r) acc += red[t][r];   // ascending rows
    a.part[(size_t)blockIdx.x * kEnergyWords + t] = acc;
  }
}

// the workgroups' partials in ascending order; T and U are half the sums of |v|^2 and phi
__global__ void __launch_bounds__(64) energy_reduce(const double* part, int groups, double* out) {
  const int q = (int)threadIdx.x;
  if (q >= kEnergyWords) return;
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += part[(size_t)g * kEnergyWords + q];
  out[q] = q <= NBODY_ENERGY_POTENTIAL ? 0.5 * s : s;
}

template <typename T, typename V4, int ARITH>
void launch_one(hipStream_t st, const EnergyArgs& a) {
  const dim3 grid((a.row_count + kEnergyRows - 1) / kEnergyRows);
  if (a.masses) hipLaunchKernelGGL((energy_kernel<T, V4, ARITH, true>), grid, dim3(kEnergyRows), 0, st, a);
  else hipLaunchKernelGGL((energy_kernel<T, V4, ARITH, false>), grid, dim3(kEnergyRows), 0, st, a);
}

}  // namespace

namespace nbl {

NBE_HIDDEN int launch_energy_kernel(int fp64, int arith, hipStream_t st, const EnergyArgs& a) {
  if (a.row_count <= 0) return 0;
  if (fp64) {   // fp64 contexts have one d2 form: REFERENCE = FMA3, REFERENCE_STRICT = STRICT
    if (arith & kStrict) launch_one<double, d4, kStrict>(st, a);
    else launch_one<double, d4, 0>(st, a);
  } else {
    switch (arith) {
      case NBODY_ARITH_REFERENCE: launch_one<float, f4, kRef>(st, a); break;
      case NBODY_ARITH_STRICT: launch_one<float, f4, kStrict>(st, a); break;
      case NBODY_ARITH_REFERENCE_STRICT: launch_one<float, f4, kRef | kStrict>(st, a); break;
      default: launch_one<float, f4, 0>(st, a); break;
    }
  }
  return (int)hipGetLastError();
}

NBE_HIDDEN int launch_energy_reduce_kernel(hipStream_t st, const double* part, int groups, double* out) {
  hipLaunchKernelGGL(energy_reduce, dim3(1), dim3(64), 0, st, part, groups, out);
  return (int)hipGetLastError();
}

}  // namespace nbl
