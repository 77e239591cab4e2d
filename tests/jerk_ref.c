/* jerk_ref.c — an independent CPU statement of the jerk of include/nbody.h ("jerk"), in its documented order:
 *   per query (x, u) and block of 1024 sources ascending, from +0 in ascending j in the context precision, d = r_j - x, w = v_j - u,
 *   inv = (|d|^2 + eps)^(-1/2), inv2 = inv * inv, inv3 = inv * inv2, rv = fma(dx, wx, fma(dy, wy, dz * wz)), c = 3 * rv, b = c * inv2,
 *   tx = fma(-b, dx, wx) (ty, tz likewise):
 *   ax = fma(dx, inv3, ax), ay, az (the field's), jx = fma(tx, inv3, jx), jy, jz;  j == skip left out;
 *   the blocks' six sums converted to binary64 and added in ascending block order from zero, each rounded once;
 *   accel = {ax, ay, az, 0}, jerk = {jx, jy, jz, 0}.  eps = the binary32 with bits 0x3089705F.
 * binary32: d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps))) or (ref) (dx*dx + dy*dy) + fmaf(dz, dz, eps), 1/sqrt as the IEEE value
 * (float)(1.0 / sqrt((double)d2)).  binary64: the fma-contracted d2, 1.0 / sqrt(d2).  Test infrastructure, compiled by the jerk tests
 * with -ffp-contract=off (products are fused only where fmaf / fma says so); queries are independent, so an OpenMP build changes no bit. */
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

/* pos, vel: n words of 4 floats; points, pvel: m words of 4 floats; skip: NULL or m ints (-1: none); ref: the reference's d2 roundings;
 * accel, jerk: m words of 4 floats each */
void jerk_f32(const float *pos, const float *vel, int n, const float *points, const float *pvel, int m, const int *skip, int ref,
              float *accel, float *jerk) {
  const float eps = eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const float x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];
    const float ux = pvel[4 * p], uy = pvel[4 * p + 1], uz = pvel[4 * p + 2];
    const int sk = skip ? skip[p] : -1;
    double l2[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      float ax = 0.0f, ay = 0.0f, az = 0.0f, jx = 0.0f, jy = 0.0f, jz = 0.0f;
      for (int j = b0; j < b1; ++j) {
        if (j == sk) continue;
        const float dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z;
        const float wx = vel[4 * j] - ux, wy = vel[4 * j + 1] - uy, wz = vel[4 * j + 2] - uz;
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
        const float rv = fmaf(dx, wx, fmaf(dy, wy, dz * wz));
        const float c = 3.0f * rv;
        const float b = c * inv2;
        const float tx = fmaf(-b, dx, wx), ty = fmaf(-b, dy, wy), tz = fmaf(-b, dz, wz);
        ax = fmaf(dx, inv3, ax);
        ay = fmaf(dy, inv3, ay);
        az = fmaf(dz, inv3, az);
        jx = fmaf(tx, inv3, jx);
        jy = fmaf(ty, inv3, jy);
        jz = fmaf(tz, inv3, jz);
      }
      l2[0] += (double)ax; l2[1] += (double)ay; l2[2] += (double)az; l2[3] += (double)jx; l2[4] += (double)jy; l2[5] += (double)jz;
    }
    float *a = accel + 4 * (size_t)p, *k = jerk + 4 * (size_t)p;
    a[0] = (float)l2[0]; a[1] = (float)l2[1]; a[2] = (float)l2[2]; a[3] = 0.0f;
    k[0] = (float)l2[3]; k[1] = (float)l2[4]; k[2] = (float)l2[5]; k[3] = 0.0f;
  }
}

/* the same with words of 4 doubles */
void jerk_f64(const double *pos, const double *vel, int n, const double *points, const double *pvel, int m, const int *skip,
              double *accel, double *jerk) {
  const double eps = (double)eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const double x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];
    const double ux = pvel[4 * p], uy = pvel[4 * p + 1], uz = pvel[4 * p + 2];
    const int sk = skip ? skip[p] : -1;
    double l2[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
      for (int j = b0; j < b1; ++j) {
        if (j == sk) continue;
        const double dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z;
        const double wx = vel[4 * j] - ux, wy = vel[4 * j + 1] - uy, wz = vel[4 * j + 2] - uz;
        const double inv = 1.0 / sqrt(fma(dx, dx, fma(dy, dy, fma(dz, dz, eps))));
        const double inv2 = inv * inv;
        const double inv3 = inv * inv2;
        const double rv = fma(dx, wx, fma(dy, wy, dz * wz));
        const double c = 3.0 * rv;
        const double b = c * inv2;
        const double tx = fma(-b, dx, wx), ty = fma(-b, dy, wy), tz = fma(-b, dz, wz);
        ax = fma(dx, inv3, ax);
        ay = fma(dy, inv3, ay);
        az = fma(dz, inv3, az);
        jx = fma(tx, inv3, jx);
        jy = fma(ty, inv3, jy);
        jz = fma(tz, inv3, jz);
      }
      l2[0] += ax; l2[1] += ay; l2[2] += az; l2[3] += jx; l2[4] += jy; l2[5] += jz;
    }
    double *a = accel + 4 * (size_t)p, *k = jerk + 4 * (size_t)p;
    a[0] = l2[0]; a[1] = l2[1]; a[2] = l2[2]; a[3] = 0.0;
    k[0] = l2[3]; k[1] = l2[4]; k[2] = l2[5]; k[3] = 0.0;
  }
}
