// energy.hip — the energy pass's device code: the all-pairs potential phi_i of every row and the per-workgroup fp64 partial sums of
// {T, U, P, L}, then one small launch that adds the partials (energy_args.hpp states the order, include/nbody.h the definitions).
// Compiles on its own; device.hip puts it into the library's one code object next to kernels.hip.  Reads nbody_args.hpp (f4, d4,
// kSoftBits) and nothing else of the force path: nbody_kernels.hpp is the force path's hashed source, so the few lines of pair
// arithmetic the potential needs are restated here, rounding for rounding.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/nbody.h"
#include "energy_args.hpp"
#include "nbody_args.hpp"

using namespace nbk;
using namespace nbe;

#define NBE_HIDDEN __attribute__((visibility("hidden")))

namespace {

constexpr int kRef = 1, kStrict = 2;   // bits of NBODY_ARITH_*: the reference's d2 roundings, the strict 1/sqrt

// 1/sqrt(|r_j - r_i|^2 + eps) with the force's d2 (nbody_kernels.hpp pair_f32): 3 v_sub, 3 v_fma (FMA3), 1 v_rsq_f32.
// Strict: the IEEE definition the library's strict 1/sqrt is proved equal to (nbody_strict_proof).
template <int ARITH>
__device__ __forceinline__ float inv_dist(float xj, float yj, float zj, float xi, float yi, float zi, float eps) {
  const float dx = xj - xi, dy = yj - yi, dz = zj - zi;
  float d2;
  if constexpr (ARITH & kRef) {
    const float sxy = dx * dx + dy * dy;             // S/dxy.vhd:113-122 (compiled with -ffp-contract=off)
    const float sz = __builtin_fmaf(dz, dz, eps);    // S/dzsoft.vhd:201-202
    d2 = sxy + sz;                                   // S/dxyz_soft.vhd:149-150
  } else {
    d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, eps)));
  }
  if constexpr (ARITH & kStrict) return (float)(1.0 / __builtin_sqrt((double)d2));
  else return __builtin_amdgcn_rsqf(d2);             // 1 ulp; d2 >= eps is never subnormal
}
// fp64 (one d2 form, as the force's pair_f64): the v_rsq_f64 seed y refined to full precision by one third-order step,
// with e = 1 - d2 y^2:  d2^(-1/2) = y (1 - e)^(-1/2) = y + y e (1/2 + 3/8 e) + O(e^3);  strict: IEEE sqrt and divide
template <int ARITH>
__device__ __forceinline__ double inv_dist(double xj, double yj, double zj, double xi, double yi, double zi, double eps) {
  const double dx = xj - xi, dy = yj - yi, dz = zj - zi;
  const double d2 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, __builtin_fma(dz, dz, eps)));
  if constexpr (ARITH & kStrict) {
    return 1.0 / __builtin_sqrt(d2);
  } else {
    const double y = __builtin_amdgcn_rsq(d2);
    const double e = __builtin_fma(-d2, y * y, 1.0);
    return __builtin_fma(y * e, __builtin_fma(e, 0.375, 0.5), y);
  }
}

template <typename T>
__device__ __forceinline__ T soft() { return (T)__builtin_bit_cast(float, kSoftBits); }   // the force's eps (S/dzsoft.vhd:177)

// One row per lane, kEnergyRows rows per workgroup, every lane walks all N sources in kEnergyBlock blocks.  Sources arrive with
// wave-uniform scalar loads (address space 4, as force_smem_f32).  The self pair is skipped by a wave-uniform branch: only the one or two
// aligned 64-source windows that overlap the wave's own 64 rows compare j with i (adding 0 in place of the self term changes no bit of a
// sum of non-negative terms); every other window is 3 sub, 3 fma, 1 rsq and 1 add per pair.
template <typename T, typename V4, int ARITH>
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
          s += inv_dist<ARITH>(p.x, p.y, p.z, me.x, me.y, me.z, eps);
        }
      } else {
#pragma unroll 8
        for (int k = 0; k < 64; ++k) {
          const V4 p = src[j + k];
          const T t = inv_dist<ARITH>(p.x, p.y, p.z, me.x, me.y, me.z, eps);
          s += (j + k == i) ? (T)0 : t;
        }
      }
    }
    for (; j < b1; ++j) {   // the last block's tail (N not a multiple of 64)
      const V4 p = src[j];
      const T t = inv_dist<ARITH>(p.x, p.y, p.z, me.x, me.y, me.z, eps);
      s += (j == i) ? (T)0 : t;
    }
    l2 += (double)s;
  }
  const double u = 0.0 - l2;                       // phi_i (N = 1: +0)
  if (a.phi && live) ((T*)a.phi)[lr - a.row0] = (T)u;
  if (!a.part) return;
  const V4 v = ((const V4*)a.vel)[live ? lr : row_end - 1];
  const double x = me.x, y = me.y, z = me.z, vx = v.x, vy = v.y, vz = v.z;
  const int t = (int)threadIdx.x;
  red[0][t] = __builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz));
  red[1][t] = u;
  red[2][t] = vx; red[3][t] = vy; red[4][t] = vz;
  red[5][t] = y * vz - z * vy;
  red[6][t] = z * vx - x * vz;
  red[7][t] = x * vy - y * vx;
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
  hipLaunchKernelGGL((energy_kernel<T, V4, ARITH>), dim3((a.row_count + kEnergyRows - 1) / kEnergyRows), dim3(kEnergyRows), 0, st, a);
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
