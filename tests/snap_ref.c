/* snap_ref.c — an independent CPU statement of the snap pass of include/nbody.h ("snap"), in its documented order:
 *   per query (x, u, g0) and block of 1024 sources ascending, from +0 in ascending j in the context precision, d = r_j - x, w = v_j - u,
 *   inv = (|d|^2 + eps)^(-1/2), inv2 = inv * inv, inv3 = inv * inv2, rv = fma(dx, wx, fma(dy, wy, dz * wz)), b = (3 * rv) * inv2,
 *   tx = fma(-b, dx, wx) (ty, tz likewise), w3 = inv3 or (mass) inv3 * m_j with m_j the w of source j's position word:
 *   ax = fma(dx, w3, ax), ay, az, jx = fma(tx, w3, jx), jy, jz                                  (the jerk pass's six);
 *   gx = axj - g0x (gy, gz), alpha = rv * inv2, q = fma(dx, gx, fma(dy, gy, fma(dz, gz, fma(wx, wx, fma(wy, wy, wz * wz))))),
 *   beta = fma(alpha, alpha, q * inv2), k6 = 6 * alpha, k3 = 3 * beta, ux = fma(-k3, dx, fma(-k6, tx, gx)) (uy, uz),
 *   sx = fma(ux, w3, sx), sy, sz;  j == skip left out;
 *   the blocks' nine sums converted to binary64 and added in ascending block order from zero, each rounded once;
 *   accel = {ax, ay, az, 0}, jerk = {jx, jy, jz, 0}, snap = {sx, sy, sz, 0}.  eps = the binary32 with bits 0x3089705F.
 * binary32: d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps))) or (ref) (dx*dx + dy*dy) + fmaf(dz, dz, eps), 1/sqrt as the IEEE value
 * (float)(1.0 / sqrt((double)d2)).  binary64: the fma-contracted d2, 1.0 / sqrt(d2).
 * The rows form (snap_rows_*): the sources' accelerations are the accel output of the same statement over all N rows (row i: query
 * (r_i, v_i), skip = i; that output does not depend on the accelerations brought), then row i's query is (r_i, v_i, a_i), skip = i.
 * Test infrastructure, compiled by the snap tests with -ffp-contract=off (products are fused only where fmaf / fma says so); queries are
 * independent, so an OpenMP build changes no bit. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define BLOCK 1024

static float eps_f32(void) {
  const uint32_t bits = 0x3089705Fu;
  float e;
  memcpy(&e, &bits, sizeof(e));
  return e;
}

static inline float inv_f32(float dx, float dy, float dz, float eps, int ref) {
  float d2;
  if (ref) {
    const float sxy = dx * dx + dy * dy;
    d2 = sxy + fmaf(dz, dz, eps);
  } else {
    d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps)));
  }
  return (float)(1.0 / sqrt((double)d2));
}

static inline double inv_f64(double dx, double dy, double dz, double eps, int ref) {
  (void)ref;
  return 1.0 / sqrt(fma(dx, dx, fma(dy, dy, fma(dz, dz, eps))));
}

/* pos, vel, acc: n words of 4 T; points, pvel, pacc: m words of 4 T; skip: NULL or m ints (-1: none); ref: the reference's d2 roundings
 * (binary32 only); mass: sources weigh the w of their position word; accel, jerk, snap: m words of 4 T each, any may be NULL */
#define SNAP(T, SUF, FMA)                                                                                                              \
  void snap_##SUF(const T *pos, const T *vel, const T *acc, int n, const T *points, const T *pvel, const T *pacc, int m,              \
                  const int *skip, int ref, int mass, T *accel, T *jerk, T *snap) {                                                   \
    const T eps = (T)eps_f32();                                                                                                        \
    _Pragma("omp parallel for schedule(dynamic, 16)")                                                                                  \
    for (int p = 0; p < m; ++p) {                                                                                                      \
      const T x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];                                                         \
      const T ux_ = pvel[4 * p], uy_ = pvel[4 * p + 1], uz_ = pvel[4 * p + 2];                                                         \
      const T g0x = pacc[4 * p], g0y = pacc[4 * p + 1], g0z = pacc[4 * p + 2];                                                         \
      const int sk = skip ? skip[p] : -1;                                                                                              \
      double l2[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };                                                                  \
      for (int b0 = 0; b0 < n; b0 += BLOCK) {                                                                                          \
        const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;                                                                                \
        T ax = 0, ay = 0, az = 0, jx = 0, jy = 0, jz = 0, sx = 0, sy = 0, sz = 0;                                                      \
        for (int j = b0; j < b1; ++j) {                                                                                                \
          if (j == sk) continue;                                                                                                       \
          const T dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z;                                               \
          const T wx = vel[4 * j] - ux_, wy = vel[4 * j + 1] - uy_, wz = vel[4 * j + 2] - uz_;                                         \
          const T inv = inv_##SUF(dx, dy, dz, eps, ref);                                                                               \
          const T inv2 = inv * inv;                                                                                                    \
          const T inv3 = inv * inv2;                                                                                                   \
          const T rv = FMA(dx, wx, FMA(dy, wy, dz * wz));                                                                              \
          const T c = (T)3 * rv;                                                                                                       \
          const T b = c * inv2;                                                                                                        \
          const T tx = FMA(-b, dx, wx), ty = FMA(-b, dy, wy), tz = FMA(-b, dz, wz);                                                    \
          const T w3 = mass ? inv3 * pos[4 * j + 3] : inv3;                                                                            \
          ax = FMA(dx, w3, ax); ay = FMA(dy, w3, ay); az = FMA(dz, w3, az);                                                            \
          jx = FMA(tx, w3, jx); jy = FMA(ty, w3, jy); jz = FMA(tz, w3, jz);                                                            \
          const T gx = acc[4 * j] - g0x, gy = acc[4 * j + 1] - g0y, gz = acc[4 * j + 2] - g0z;                                         \
          const T alpha = rv * inv2;                                                                                                   \
          const T q = FMA(dx, gx, FMA(dy, gy, FMA(dz, gz, FMA(wx, wx, FMA(wy, wy, wz * wz)))));                                        \
          const T qi = q * inv2;                                                                                                       \
          const T beta = FMA(alpha, alpha, qi);                                                                                        \
          const T k6 = (T)6 * alpha, k3 = (T)3 * beta;                                                                                 \
          const T ux = FMA(-k3, dx, FMA(-k6, tx, gx)), uy = FMA(-k3, dy, FMA(-k6, ty, gy)), uz = FMA(-k3, dz, FMA(-k6, tz, gz));       \
          sx = FMA(ux, w3, sx); sy = FMA(uy, w3, sy); sz = FMA(uz, w3, sz);                                                            \
        }                                                                                                                              \
        l2[0] += (double)ax; l2[1] += (double)ay; l2[2] += (double)az; l2[3] += (double)jx; l2[4] += (double)jy; l2[5] += (double)jz;  \
        l2[6] += (double)sx; l2[7] += (double)sy; l2[8] += (double)sz;                                                                 \
      }                                                                                                                                \
      T *out[3] = { accel, jerk, snap };                                                                                               \
      for (int o = 0; o < 3; ++o)                                                                                                      \
        if (out[o]) {                                                                                                                  \
          T *w = out[o] + 4 * (size_t)p;                                                                                               \
          w[0] = (T)l2[3 * o]; w[1] = (T)l2[3 * o + 1]; w[2] = (T)l2[3 * o + 2]; w[3] = (T)0;                                          \
        }                                                                                                                              \
    }                                                                                                                                  \
  }                                                                                                                                    \
  /* the rows form over all n rows: two passes */                                                                                     \
  void snap_rows_##SUF(const T *pos, const T *vel, int n, int ref, int mass, T *accel, T *jerk, T *snap) {                             \
    int *self = (int *)malloc(sizeof(int) * (size_t)n);                                                                                \
    T *a = (T *)calloc(4 * (size_t)n, sizeof(T)), *zero = (T *)calloc(4 * (size_t)n, sizeof(T));                                       \
    for (int i = 0; i < n; ++i) self[i] = i;                                                                                           \
    snap_##SUF(pos, vel, zero, n, pos, vel, zero, n, self, ref, mass, a, NULL, NULL);                                                  \
    snap_##SUF(pos, vel, a, n, pos, vel, a, n, self, ref, mass, accel, jerk, snap);                                                    \
    free(self); free(a); free(zero);                                                                                                   \
  }

SNAP(float, f32, fmaf)
SNAP(double, f64, fma)
