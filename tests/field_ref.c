/* field_ref.c — an independent CPU statement of the field of include/nbody.h ("field at arbitrary points"), in its documented order:
 *   per point x and block of 1024 sources ascending: ax = fma(dx, inv3, ax) (ay, az likewise), s = s + inv from +0 in ascending j in
 *   the context precision, d = r_j - x, inv = (|d|^2 + eps)^(-1/2), inv3 = inv * (inv * inv), j == skip left out; the blocks' four sums
 *   converted to binary64 and added in ascending block order from zero; accel = (T){A}, w = 0; phi = (T)(0 - S).
 *   eps = the binary32 with bits 0x3089705F.
 * binary32: d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps))) or (ref) (dx*dx + dy*dy) + fmaf(dz, dz, eps), 1/sqrt as the IEEE value
 * (float)(1.0 / sqrt((double)d2)).  binary64: the fma-contracted d2, 1.0 / sqrt(d2).  Test infrastructure, compiled by the field tests
 * with -ffp-contract=off (products are fused only where fmaf / fma says so); points are independent, so an OpenMP build changes no bit. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define BLOCK 1024

static float eps_f32(void) {
  const uint32_t bits = 0x3089705Fu;
  float e;
  memcpy(&e, &bits, sizeof(e));
  return e;
}

/* pos: n words of 4 floats; points: m words of 4 floats; skip: NULL or m ints (-1: none); ref: the reference's d2 roundings;
 * accel: m words {ax, ay, az, 0} or NULL; phi: m values or NULL */
void field_f32(const float *pos, int n, const float *points, int m, const int *skip, int ref, float *accel, float *phi) {
  const float eps = eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const float x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];
    const int sk = skip ? skip[p] : -1;
    double a2x = 0.0, a2y = 0.0, a2z = 0.0, s2 = 0.0;
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      float ax = 0.0f, ay = 0.0f, az = 0.0f, s1 = 0.0f;
      for (int j = b0; j < b1; ++j) {
        if (j == sk) continue;
        const float dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z;
        float d2;
        if (ref) {
          const float sxy = dx * dx + dy * dy;
          d2 = sxy + fmaf(dz, dz, eps);
        } else {
          d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps)));
        }
        const float inv = (float)(1.0 / sqrt((double)d2));
        const float inv2 = inv * inv;
        const float inv3 = inv * inv2;
        ax = fmaf(dx, inv3, ax);
        ay = fmaf(dy, inv3, ay);
        az = fmaf(dz, inv3, az);
        s1 += inv;
      }
      a2x += (double)ax; a2y += (double)ay; a2z += (double)az; s2 += (double)s1;
    }
    if (accel) {
      accel[4 * p] = (float)a2x; accel[4 * p + 1] = (float)a2y; accel[4 * p + 2] = (float)a2z; accel[4 * p + 3] = 0.0f;
    }
    if (phi) phi[p] = (float)(0.0 - s2);
  }
}

/* the same with words of 4 doubles */
void field_f64(const double *pos, int n, const double *points, int m, const int *skip, double *accel, double *phi) {
  const double eps = (double)eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const double x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];
    const int sk = skip ? skip[p] : -1;
    double a2x = 0.0, a2y = 0.0, a2z = 0.0, s2 = 0.0;
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      double ax = 0.0, ay = 0.0, az = 0.0, s1 = 0.0;
      for (int j = b0; j < b1; ++j) {
        if (j == sk) continue;
        const double dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z;
        const double inv = 1.0 / sqrt(fma(dx, dx, fma(dy, dy, fma(dz, dz, eps))));
        const double inv2 = inv * inv;
        const double inv3 = inv * inv2;
        ax = fma(dx, inv3, ax);
        ay = fma(dy, inv3, ay);
        az = fma(dz, inv3, az);
        s1 += inv;
      }
      a2x += ax; a2y += ay; a2z += az; s2 += s1;
    }
    if (accel) {
      accel[4 * p] = a2x; accel[4 * p + 1] = a2y; accel[4 * p + 2] = a2z; accel[4 * p + 3] = 0.0;
    }
    if (phi) phi[p] = 0.0 - s2;
  }
}
