/* tidal_ref.c — an independent CPU statement of the tidal tensor of include/nbody.h ("tidal tensor at arbitrary points"), in its
 * documented order:
 *   per point x and block of 1024 sources ascending, from +0 in ascending j in the context precision, d = r_j - x,
 *   inv = (|d|^2 + eps)^(-1/2), inv2 = inv * inv, inv3 = inv * inv2, inv5 = inv3 * inv2, w = 3 * inv5, wx = w * dx (wy, wz likewise):
 *   qxx = fma(wx, dx, qxx), qyy, qzz, qxy = fma(wx, dy, qxy), qxz = fma(wx, dz, qxz), qyz = fma(wy, dz, qyz), s3 = s3 + inv3,
 *   j == skip left out; the blocks' seven sums converted to binary64 and added in ascending block order from zero;
 *   T_aa = (T)(Q_aa - S3), T_ab = (T)Q_ab, six values per point {xx, yy, zz, xy, xz, yz}.  eps = the binary32 with bits 0x3089705F.
 * binary32: d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps))) or (ref) (dx*dx + dy*dy) + fmaf(dz, dz, eps), 1/sqrt as the IEEE value
 * (float)(1.0 / sqrt((double)d2)).  binary64: the fma-contracted d2, 1.0 / sqrt(d2).  Test infrastructure, compiled by the tidal tests
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
 * tensor: m x 6 values */
void tidal_f32(const float *pos, int n, const float *points, int m, const int *skip, int ref, float *tensor) {
  const float eps = eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const float x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];
    const int sk = skip ? skip[p] : -1;
    double q2[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, s2 = 0.0;
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      float xx = 0.0f, yy = 0.0f, zz = 0.0f, xy = 0.0f, xz = 0.0f, yz = 0.0f, s3 = 0.0f;
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
        const float inv5 = inv3 * inv2;
        const float w = 3.0f * inv5;
        const float wx = w * dx, wy = w * dy, wz = w * dz;
        xx = fmaf(wx, dx, xx);
        yy = fmaf(wy, dy, yy);
        zz = fmaf(wz, dz, zz);
        xy = fmaf(wx, dy, xy);
        xz = fmaf(wx, dz, xz);
        yz = fmaf(wy, dz, yz);
        s3 += inv3;
      }
      q2[0] += (double)xx; q2[1] += (double)yy; q2[2] += (double)zz; q2[3] += (double)xy; q2[4] += (double)xz; q2[5] += (double)yz;
      s2 += (double)s3;
    }
    float *t = tensor + 6 * (size_t)p;
    t[0] = (float)(q2[0] - s2); t[1] = (float)(q2[1] - s2); t[2] = (float)(q2[2] - s2);
    t[3] = (float)q2[3]; t[4] = (float)q2[4]; t[5] = (float)q2[5];
  }
}

/* the same with words of 4 doubles */
void tidal_f64(const double *pos, int n, const double *points, int m, const int *skip, double *tensor) {
  const double eps = (double)eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const double x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];
    const int sk = skip ? skip[p] : -1;
    double q2[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, s2 = 0.0;
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      double xx = 0.0, yy = 0.0, zz = 0.0, xy = 0.0, xz = 0.0, yz = 0.0, s3 = 0.0;
      for (int j = b0; j < b1; ++j) {
        if (j == sk) continue;
        const double dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z;
        const double inv = 1.0 / sqrt(fma(dx, dx, fma(dy, dy, fma(dz, dz, eps))));
        const double inv2 = inv * inv;
        const double inv3 = inv * inv2;
        const double inv5 = inv3 * inv2;
        const double w = 3.0 * inv5;
        const double wx = w * dx, wy = w * dy, wz = w * dz;
        xx = fma(wx, dx, xx);
        yy = fma(wy, dy, yy);
        zz = fma(wz, dz, zz);
        xy = fma(wx, dy, xy);
        xz = fma(wx, dz, xz);
        yz = fma(wy, dz, yz);
        s3 += inv3;
      }
      q2[0] += xx; q2[1] += yy; q2[2] += zz; q2[3] += xy; q2[4] += xz; q2[5] += yz;
      s2 += s3;
    }
    double *t = tensor + 6 * (size_t)p;
    t[0] = q2[0] - s2; t[1] = q2[1] - s2; t[2] = q2[2] - s2;
    t[3] = q2[3]; t[4] = q2[4]; t[5] = q2[5];
  }
}
