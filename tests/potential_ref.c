/* potential_ref.c — an independent CPU statement of the potential of include/nbody.h ("energy and potential"), in its documented order:
 *   phi_i = 0 - S_i,  S_i = sum over blocks of 1024 sources ascending (fp64) of the block's sum from zero, ascending j, j != i, of
 *   (|r_j - r_i|^2 + eps)^(-1/2) in the context precision;  eps = the binary32 with bits 0x3089705F.
 * binary32: d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps))) or (ref) (dx*dx + dy*dy) + fmaf(dz, dz, eps), 1/sqrt as the IEEE value
 * (float)(1.0 / sqrt((double)d2)).  binary64: the fma-contracted d2, 1.0 / sqrt(d2).  Test infrastructure, compiled by
 * tests/test_gpu_energy.py with -ffp-contract=off (products are fused only where fmaf / fma says so); rows are independent, so an
 * OpenMP build changes no bit. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define BLOCK 1024

static float eps_f32(void) {
  const uint32_t bits = 0x3089705Fu;
  float e;
  memcpy(&e, &bits, sizeof(e));
  return e;
}

/* pos: n words of 4 floats; phi[k] = phi of row r0 + k, k < nr; ref: the reference's d2 roundings */
void potential_f32(const float *pos, int n, int r0, int nr, int ref, float *phi) {
  const float eps = eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int k = 0; k < nr; ++k) {
    const int i = r0 + k;
    const float xi = pos[4 * i], yi = pos[4 * i + 1], zi = pos[4 * i + 2];
    double s2 = 0.0;
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      float s1 = 0.0f;
      for (int j = b0; j < b1; ++j) {
        if (j == i) continue;
        const float dx = pos[4 * j] - xi, dy = pos[4 * j + 1] - yi, dz = pos[4 * j + 2] - zi;
        float d2;
        if (ref) {
          const float sxy = dx * dx + dy * dy;
          d2 = sxy + fmaf(dz, dz, eps);
        } else {
          d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps)));
        }
        s1 += (float)(1.0 / sqrt((double)d2));
      }
      s2 += (double)s1;
    }
    phi[k] = (float)(0.0 - s2);
  }
}

/* pos: n words of 4 doubles */
void potential_f64(const double *pos, int n, int r0, int nr, double *phi) {
  const double eps = (double)eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int k = 0; k < nr; ++k) {
    const int i = r0 + k;
    const double xi = pos[4 * i], yi = pos[4 * i + 1], zi = pos[4 * i + 2];
    double s2 = 0.0;
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      double s1 = 0.0;
      for (int j = b0; j < b1; ++j) {
        if (j == i) continue;
        const double dx = pos[4 * j] - xi, dy = pos[4 * j + 1] - yi, dz = pos[4 * j + 2] - zi;
        s1 += 1.0 / sqrt(fma(dx, dx, fma(dy, dy, fma(dz, dz, eps))));
      }
      s2 += s1;
    }
    phi[k] = 0.0 - s2;
  }
}
