/* masses_ref.c — an independent CPU statement of the passes of include/nbody.h "with NBODY_OPT_MASSES": body j weighs m_j = the fourth
 * value of its position word.  The order is the documented one of every pass — per query and block of 1024 sources ascending, from +0 in
 * ascending j in the precision T of the words, j == skip left out; the blocks' sums converted to binary64 and added in ascending block
 * order from zero, each result rounded once — and the pair, with d = r_j - x, inv = (|d|^2 + eps)^(-1/2), inv2 = inv * inv, inv3 = inv * inv2,
 * m = m_j, takes ONE more rounding than the unweighted pair of field_ref.c, tidal_ref.c, jerk_ref.c and potential_ref.c:
 *   field      w3 = m * inv3;  ax = fma(dx, w3, ax), ay, az;  s = fma(m, inv, s);                accel = {ax, ay, az, 0}, phi = 0 - s
 *   jerk       w3 = m * inv3;  the field's ax, ay, az;  w = v_j - u, rv = fma(dx, wx, fma(dy, wy, dz * wz)), b = (3 * rv) * inv2,
 *              tx = fma(-b, dx, wx) (ty, tz);  jx = fma(tx, w3, jx), jy, jz
 *   tidal      inv5 = inv3 * inv2, w = (3 * inv5) * m, wx = w * dx (wy, wz);  qxx = fma(wx, dx, qxx), qyy, qzz, qxy = fma(wx, dy, qxy),
 *              qxz = fma(wx, dz, qxz), qyz = fma(wy, dz, qyz);  s3 = fma(m, inv3, s3);  T_aa = Q_aa - S3, T_ab = Q_ab
 *   potential  s = fma(m, inv, s), j == i left out;  phi_i = 0 - S_i
 *   totals     potential_ref.c's groups and slices, a row's eight binary64 terms each times mi = (double)m_i (one binary64 product more)
 * binary32: d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps))) or (ref) (dx*dx + dy*dy) + fmaf(dz, dz, eps), 1/sqrt as the IEEE value
 * (float)(1.0 / sqrt((double)d2)).  binary64: the fma-contracted d2, 1.0 / sqrt(d2); ref is ignored.  eps = the binary32 0x3089705F.
 * The Hermite shared-step and block-step loops restate hermite_ref.c and hermite_block_ref.c on this jerk: the acceleration and the jerk
 * are per unit mass of the row, so predictor, corrector, level rule and counters are theirs, and the fourth value of a position word is
 * carried.  Test infrastructure, compiled with -ffp-contract=off (products are fused only where fmaf / fma says so); queries are
 * independent, so an OpenMP build changes no bit. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define BLOCK 1024
#define GROUP 256
#define WORDS 8

static float eps_f32(void) {
  const uint32_t bits = 0x3089705Fu;
  float e;
  memcpy(&e, &bits, sizeof(e));
  return e;
}

static float inv_f32(float dx, float dy, float dz, float eps, int ref) {
  float d2;
  if (ref) {
    const float sxy = dx * dx + dy * dy;
    d2 = sxy + fmaf(dz, dz, eps);
  } else {
    d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps)));
  }
  return (float)(1.0 / sqrt((double)d2));
}
static double inv_f64(double dx, double dy, double dz, double eps, int ref) {
  (void)ref;
  return 1.0 / sqrt(fma(dx, dx, fma(dy, dy, fma(dz, dz, eps))));
}

#define PASSES(T, SUF, FMA)                                                                                                           \
  /* pos: n words; points: m words; skip: NULL or m ints (-1: none); accel: m words or NULL; phi: m values or NULL */                 \
  void m_field_##SUF(const T *pos, int n, const T *points, int m, const int *skip, int ref, T *accel, T *phi) {                       \
    const T eps = (T)eps_f32();                                                                                                       \
    _Pragma("omp parallel for schedule(dynamic, 16)")                                                                                 \
    for (int p = 0; p < m; ++p) {                                                                                                     \
      const T x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];                                                        \
      const int sk = skip ? skip[p] : -1;                                                                                             \
      double l2[4] = { 0.0, 0.0, 0.0, 0.0 };                                                                                          \
      for (int b0 = 0; b0 < n; b0 += BLOCK) {                                                                                         \
        const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;                                                                               \
        T ax = 0, ay = 0, az = 0, s = 0;                                                                                              \
        for (int j = b0; j < b1; ++j) {                                                                                               \
          if (j == sk) continue;                                                                                                      \
          const T dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z, mj = pos[4 * j + 3];                         \
          const T inv = inv_##SUF(dx, dy, dz, eps, ref);                                                                              \
          const T inv2 = inv * inv;                                                                                                   \
          const T inv3 = inv * inv2;                                                                                                  \
          const T w3 = mj * inv3;                                                                                                     \
          ax = FMA(dx, w3, ax); ay = FMA(dy, w3, ay); az = FMA(dz, w3, az);                                                           \
          s = FMA(mj, inv, s);                                                                                                        \
        }                                                                                                                             \
        l2[0] += (double)ax; l2[1] += (double)ay; l2[2] += (double)az; l2[3] += (double)s;                                            \
      }                                                                                                                               \
      if (accel) { T *a = accel + 4 * (size_t)p; a[0] = (T)l2[0]; a[1] = (T)l2[1]; a[2] = (T)l2[2]; a[3] = 0; }                       \
      if (phi) phi[p] = (T)(0.0 - l2[3]);                                                                                             \
    }                                                                                                                                 \
  }                                                                                                                                   \
  /* tensor: m x 6 values {xx, yy, zz, xy, xz, yz} */                                                                                 \
  void m_tidal_##SUF(const T *pos, int n, const T *points, int m, const int *skip, int ref, T *tensor) {                              \
    const T eps = (T)eps_f32();                                                                                                       \
    _Pragma("omp parallel for schedule(dynamic, 16)")                                                                                 \
    for (int p = 0; p < m; ++p) {                                                                                                     \
      const T x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];                                                        \
      const int sk = skip ? skip[p] : -1;                                                                                             \
      double l2[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };                                                                           \
      for (int b0 = 0; b0 < n; b0 += BLOCK) {                                                                                         \
        const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;                                                                               \
        T c[7] = { 0, 0, 0, 0, 0, 0, 0 };                                                                                             \
        for (int j = b0; j < b1; ++j) {                                                                                               \
          if (j == sk) continue;                                                                                                      \
          const T dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z, mj = pos[4 * j + 3];                         \
          const T inv = inv_##SUF(dx, dy, dz, eps, ref);                                                                              \
          const T inv2 = inv * inv;                                                                                                   \
          const T inv3 = inv * inv2;                                                                                                  \
          const T inv5 = inv3 * inv2;                                                                                                 \
          const T w0 = (T)3 * inv5;                                                                                                   \
          const T w = w0 * mj;                                                                                                        \
          const T wx = w * dx, wy = w * dy, wz = w * dz;                                                                              \
          c[0] = FMA(wx, dx, c[0]); c[1] = FMA(wy, dy, c[1]); c[2] = FMA(wz, dz, c[2]);                                               \
          c[3] = FMA(wx, dy, c[3]); c[4] = FMA(wx, dz, c[4]); c[5] = FMA(wy, dz, c[5]);                                               \
          c[6] = FMA(mj, inv3, c[6]);                                                                                                 \
        }                                                                                                                             \
        for (int q = 0; q < 7; ++q) l2[q] += (double)c[q];                                                                            \
      }                                                                                                                               \
      T *t = tensor + 6 * (size_t)p;                                                                                                  \
      t[0] = (T)(l2[0] - l2[6]); t[1] = (T)(l2[1] - l2[6]); t[2] = (T)(l2[2] - l2[6]);                                                \
      t[3] = (T)l2[3]; t[4] = (T)l2[4]; t[5] = (T)l2[5];                                                                              \
    }                                                                                                                                 \
  }                                                                                                                                   \
  /* pos, vel: n words; points, pvel: m words; accel, jerk: m words each */                                                           \
  void m_jerk_##SUF(const T *pos, const T *vel, int n, const T *points, const T *pvel, int m, const int *skip, int ref, T *accel,     \
                    T *jerk) {                                                                                                        \
    const T eps = (T)eps_f32();                                                                                                       \
    _Pragma("omp parallel for schedule(dynamic, 16)")                                                                                 \
    for (int p = 0; p < m; ++p) {                                                                                                     \
      const T x = points[4 * p], y = points[4 * p + 1], z = points[4 * p + 2];                                                        \
      const T ux = pvel[4 * p], uy = pvel[4 * p + 1], uz = pvel[4 * p + 2];                                                           \
      const int sk = skip ? skip[p] : -1;                                                                                             \
      double l2[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };                                                                                \
      for (int b0 = 0; b0 < n; b0 += BLOCK) {                                                                                         \
        const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;                                                                               \
        T ax = 0, ay = 0, az = 0, jx = 0, jy = 0, jz = 0;                                                                             \
        for (int j = b0; j < b1; ++j) {                                                                                               \
          if (j == sk) continue;                                                                                                      \
          const T dx = pos[4 * j] - x, dy = pos[4 * j + 1] - y, dz = pos[4 * j + 2] - z, mj = pos[4 * j + 3];                         \
          const T wx = vel[4 * j] - ux, wy = vel[4 * j + 1] - uy, wz = vel[4 * j + 2] - uz;                                           \
          const T inv = inv_##SUF(dx, dy, dz, eps, ref);                                                                              \
          const T inv2 = inv * inv;                                                                                                   \
          const T inv3 = inv * inv2;                                                                                                  \
          const T rv = FMA(dx, wx, FMA(dy, wy, dz * wz));                                                                             \
          const T c = (T)3 * rv;                                                                                                      \
          const T b = c * inv2;                                                                                                       \
          const T tx = FMA(-b, dx, wx), ty = FMA(-b, dy, wy), tz = FMA(-b, dz, wz);                                                   \
          const T w3 = mj * inv3;                                                                                                     \
          ax = FMA(dx, w3, ax); ay = FMA(dy, w3, ay); az = FMA(dz, w3, az);                                                           \
          jx = FMA(tx, w3, jx); jy = FMA(ty, w3, jy); jz = FMA(tz, w3, jz);                                                           \
        }                                                                                                                             \
        l2[0] += (double)ax; l2[1] += (double)ay; l2[2] += (double)az; l2[3] += (double)jx; l2[4] += (double)jy; l2[5] += (double)jz; \
      }                                                                                                                               \
      T *a = accel + 4 * (size_t)p, *k = jerk + 4 * (size_t)p;                                                                        \
      a[0] = (T)l2[0]; a[1] = (T)l2[1]; a[2] = (T)l2[2]; a[3] = 0;                                                                    \
      k[0] = (T)l2[3]; k[1] = (T)l2[4]; k[2] = (T)l2[5]; k[3] = 0;                                                                    \
    }                                                                                                                                 \
  }                                                                                                                                   \
  /* S_i in binary64, before phi_i = 0 - S_i is rounded to T */                                                                       \
  static double m_s_row_##SUF(const T *pos, int n, int i, int ref) {                                                                  \
    const T eps = (T)eps_f32();                                                                                                       \
    const T xi = pos[4 * i], yi = pos[4 * i + 1], zi = pos[4 * i + 2];                                                                \
    double s2 = 0.0;                                                                                                                  \
    for (int b0 = 0; b0 < n; b0 += BLOCK) {                                                                                           \
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;                                                                                 \
      T s1 = 0;                                                                                                                       \
      for (int j = b0; j < b1; ++j) {                                                                                                 \
        if (j == i) continue;                                                                                                         \
        const T dx = pos[4 * j] - xi, dy = pos[4 * j + 1] - yi, dz = pos[4 * j + 2] - zi;                                             \
        s1 = FMA(pos[4 * j + 3], inv_##SUF(dx, dy, dz, eps, ref), s1);                                                                \
      }                                                                                                                               \
      s2 += (double)s1;                                                                                                               \
    }                                                                                                                                 \
    return s2;                                                                                                                        \
  }                                                                                                                                   \
  /* phi[k] = phi of row r0 + k, k < nr */                                                                                            \
  void m_potential_##SUF(const T *pos, int n, int r0, int nr, int ref, T *phi) {                                                      \
    _Pragma("omp parallel for schedule(dynamic, 16)")                                                                                 \
    for (int k = 0; k < nr; ++k) phi[k] = (T)(0.0 - m_s_row_##SUF(pos, n, r0 + k, ref));                                              \
  }                                                                                                                                   \
  /* slices: nslices pairs {first, count}; out: 8 values; returns 0, or 1 without memory */                                           \
  int m_energy_totals_##SUF(const T *pos, const T *vel, int n, const int *slices, int nslices, int ref, double *out) {                \
    double *w = (double *)malloc((size_t)n * WORDS * sizeof(double));                                                                 \
    if (!w) return 1;                                                                                                                 \
    _Pragma("omp parallel for schedule(dynamic, 16)")                                                                                 \
    for (int i = 0; i < n; ++i) {                                                                                                     \
      const double u = 0.0 - m_s_row_##SUF(pos, n, i, ref), mi = (double)pos[4 * i + 3];                                              \
      const double x = pos[4 * i], y = pos[4 * i + 1], z = pos[4 * i + 2], vx = vel[4 * i], vy = vel[4 * i + 1], vz = vel[4 * i + 2]; \
      double *r = w + (size_t)WORDS * i;                                                                                              \
      const double v2 = fma(vx, vx, fma(vy, vy, vz * vz));                                                                            \
      const double yvz = y * vz, zvy = z * vy, zvx = z * vx, xvz = x * vz, xvy = x * vy, yvx = y * vx;                                \
      const double lx = yvz - zvy, ly = zvx - xvz, lz = xvy - yvx;                                                                    \
      r[0] = mi * v2; r[1] = mi * u; r[2] = mi * vx; r[3] = mi * vy; r[4] = mi * vz; r[5] = mi * lx; r[6] = mi * ly; r[7] = mi * lz;  \
    }                                                                                                                                 \
    for (int q = 0; q < WORDS; ++q) out[q] = 0.0;                                                                                     \
    for (int r = 0; r < nslices; ++r) {                                                                                               \
      const int first = slices[2 * r], end = first + slices[2 * r + 1];                                                               \
      double tot[WORDS] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };                                                                 \
      for (int g0 = first; g0 < end; g0 += GROUP) {                                                                                   \
        const int g1 = g0 + GROUP < end ? g0 + GROUP : end;                                                                           \
        double acc[WORDS] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };                                                               \
        for (int i = g0; i < g1; ++i)                                                                                                 \
          for (int q = 0; q < WORDS; ++q) acc[q] += w[(size_t)WORDS * i + q];                                                         \
        for (int q = 0; q < WORDS; ++q) tot[q] += acc[q];                                                                             \
      }                                                                                                                               \
      tot[0] = 0.5 * tot[0];                                                                                                          \
      tot[1] = 0.5 * tot[1];                                                                                                          \
      for (int q = 0; q < WORDS; ++q) out[q] += tot[q];                                                                               \
    }                                                                                                                                 \
    free(w);                                                                                                                          \
    return 0;                                                                                                                         \
  }                                                                                                                                   \
  /* hermite_ref.c's call of nsteps steps of dt, in place, on the weighted jerk: (a0, j0) of every row (skip = self), then per step  \
   * predict, evaluate at the predicted state, correct; the fourth values are carried */                                             \
  void m_hermite_##SUF(T *pos, T *vel, int n, T dt, int nsteps, int ref) {                                                            \
    const size_t words = 4 * (size_t)n;                                                                                               \
    int *self = (int *)malloc(sizeof(int) * (size_t)n);                                                                               \
    T *a[2], *j[2], *x0 = (T *)malloc(sizeof(T) * words), *v0 = (T *)malloc(sizeof(T) * words);                                       \
    int k = 0;                                                                                                                        \
    for (int i = 0; i < n; ++i) self[i] = i;                                                                                          \
    for (int q = 0; q < 2; ++q) { a[q] = (T *)malloc(sizeof(T) * words); j[q] = (T *)malloc(sizeof(T) * words); }                     \
    m_jerk_##SUF(pos, vel, n, pos, vel, n, self, ref, a[0], j[0]);                                                                    \
    const T h = dt, h2 = h * h, c2 = h2 * (T)0.5, h3 = h2 * h, c3 = h3 / (T)6, hh = h * (T)0.5, c12 = h2 / (T)12;                     \
    for (int s = 0; s < nsteps; ++s) {                                                                                                \
      const T *a0 = a[k], *j0 = j[k];                                                                                                 \
      T *a1 = a[k ^ 1], *j1 = j[k ^ 1];                                                                                               \
      memcpy(x0, pos, sizeof(T) * words);                                                                                             \
      memcpy(v0, vel, sizeof(T) * words);                                                                                             \
      for (int i = 0; i < n; ++i)                                                                                                     \
        for (int c = 0; c < 3; ++c) {                                                                                                 \
          const size_t e = 4 * (size_t)i + c;                                                                                         \
          pos[e] = FMA(c3, j0[e], FMA(c2, a0[e], FMA(h, v0[e], x0[e])));                                                              \
          vel[e] = FMA(c2, j0[e], FMA(h, a0[e], v0[e]));                                                                              \
        }                                                                                                                             \
      m_jerk_##SUF(pos, vel, n, pos, vel, n, self, ref, a1, j1);                                                                      \
      for (int i = 0; i < n; ++i)                                                                                                     \
        for (int c = 0; c < 3; ++c) {                                                                                                 \
          const size_t e = 4 * (size_t)i + c;                                                                                         \
          const T dj = j0[e] - j1[e], sa = a0[e] + a1[e], da = a0[e] - a1[e];                                                         \
          const T v1 = FMA(c12, dj, FMA(hh, sa, v0[e]));                                                                              \
          const T sv = v0[e] + v1;                                                                                                    \
          vel[e] = v1;                                                                                                                \
          pos[e] = FMA(c12, da, FMA(hh, sv, x0[e]));                                                                                  \
        }                                                                                                                             \
      k ^= 1;                                                                                                                         \
    }                                                                                                                                 \
    free(self); free(x0); free(v0);                                                                                                   \
    for (int q = 0; q < 2; ++q) { free(a[q]); free(j[q]); }                                                                           \
  }                                                                                                                                   \
  static int m_want_##SUF(const T *a, const T *j, double eta2, const double *lim, int levels) {                                       \
    const double ax = (double)a[0], ay = (double)a[1], az = (double)a[2], jx = (double)j[0], jy = (double)j[1], jz = (double)j[2];    \
    const double a2 = (ax * ax + ay * ay) + az * az, j2 = (jx * jx + jy * jy) + jz * jz;                                              \
    const double q = a2 / j2;                                                                                                         \
    if (!(q < INFINITY)) return 0;                                                                                                    \
    const double e = eta2 * q;                                                                                                        \
    for (int k = 0; k < levels; ++k)                                                                                                  \
      if (lim[k] <= e) return k;                                                                                                      \
    return levels - 1;                                                                                                                \
  }                                                                                                                                   \
  /* hermite_block_ref.c's call on the weighted jerk at points, in place; returns 0, or a negative value where the invariant fails */ \
  int m_hermite_block_##SUF(T *pos, T *vel, int n, int ref, T eta, T dt_max, int levels, int nblocks, long long *substeps,            \
                            long long *row_evals) {                                                                                   \
    const size_t words = 4 * (size_t)n;                                                                                               \
    const T unit = (T)ldexp((double)dt_max, -(levels - 1));                                                                           \
    const double eta2 = (double)eta * (double)eta;                                                                                    \
    double lim[64];                                                                                                                   \
    for (int k = 0; k < levels; ++k) { const double dk = ldexp((double)dt_max, -k); lim[k] = dk * dk; }                               \
    T *x0 = (T *)malloc(sizeof(T) * words), *v0 = (T *)malloc(sizeof(T) * words), *a0 = (T *)malloc(sizeof(T) * words);               \
    T *j0 = (T *)malloc(sizeof(T) * words), *a1 = (T *)malloc(sizeof(T) * words), *j1 = (T *)malloc(sizeof(T) * words);               \
    T *pts = (T *)malloc(sizeof(T) * words), *pv = (T *)malloc(sizeof(T) * words);                                                    \
    long long *t0 = (long long *)calloc((size_t)n, sizeof(long long));                                                                \
    int *lev = (int *)malloc(sizeof(int) * (size_t)n), *act = (int *)malloc(sizeof(int) * (size_t)n);                                 \
    const long long end = (long long)nblocks << (levels - 1);                                                                         \
    long long steps = 0, evals = 0, tau = 0;                                                                                          \
    int rc = 0;                                                                                                                       \
    memcpy(x0, pos, sizeof(T) * words);                                                                                               \
    memcpy(v0, vel, sizeof(T) * words);                                                                                               \
    for (int i = 0; i < n; ++i) act[i] = i;                                                                                           \
    m_jerk_##SUF(pos, vel, n, pos, vel, n, act, ref, a0, j0);                                                                         \
    for (int i = 0; i < n; ++i) lev[i] = m_want_##SUF(a0 + 4 * (size_t)i, j0 + 4 * (size_t)i, eta2, lim, levels);                     \
    while (tau < end && rc == 0) {                                                                                                    \
      int m = 0;                                                                                                                      \
      tau = t0[0] + (1LL << (levels - 1 - lev[0]));                                                                                   \
      for (int i = 1; i < n; ++i) { const long long nx = t0[i] + (1LL << (levels - 1 - lev[i])); if (nx < tau) tau = nx; }            \
      if (tau > end) { rc = -1; break; }                                                                                              \
      for (int i = 0; i < n; ++i) {                                                                                                   \
        const long long s = 1LL << (levels - 1 - lev[i]);                                                                             \
        if (t0[i] % s != 0) rc = -2;                                                                                                  \
        if (t0[i] + s == tau) act[m++] = i;                                                                                           \
        const T h = (T)(tau - t0[i]) * unit;                                                                                          \
        const T h2 = h * h, c2 = h2 * (T)0.5, h3 = h2 * h, c3 = h3 / (T)6;                                                            \
        for (int c = 0; c < 3; ++c) {                                                                                                 \
          const size_t e = 4 * (size_t)i + c;                                                                                         \
          pos[e] = FMA(c3, j0[e], FMA(c2, a0[e], FMA(h, v0[e], x0[e])));                                                              \
          vel[e] = FMA(c2, j0[e], FMA(h, a0[e], v0[e]));                                                                              \
        }                                                                                                                             \
        pos[4 * (size_t)i + 3] = x0[4 * (size_t)i + 3];                                                                               \
        vel[4 * (size_t)i + 3] = v0[4 * (size_t)i + 3];                                                                               \
      }                                                                                                                               \
      for (int q = 0; q < m; ++q) {                                                                                                   \
        memcpy(pts + 4 * (size_t)q, pos + 4 * (size_t)act[q], sizeof(T) * 4);                                                         \
        memcpy(pv + 4 * (size_t)q, vel + 4 * (size_t)act[q], sizeof(T) * 4);                                                          \
      }                                                                                                                               \
      m_jerk_##SUF(pos, vel, n, pts, pv, m, act, ref, a1, j1);                                                                        \
      for (int q = 0; q < m; ++q) {                                                                                                   \
        const int i = act[q];                                                                                                         \
        const T h = (T)(tau - t0[i]) * unit;                                                                                          \
        const T h2 = h * h, hh = h * (T)0.5, c12 = h2 / (T)12;                                                                        \
        for (int c = 0; c < 3; ++c) {                                                                                                 \
          const size_t e = 4 * (size_t)i + c, f = 4 * (size_t)q + c;                                                                  \
          const T dj = j0[e] - j1[f], sa = a0[e] + a1[f], da = a0[e] - a1[f];                                                         \
          const T w1 = FMA(c12, dj, FMA(hh, sa, v0[e]));                                                                              \
          const T sv = v0[e] + w1;                                                                                                    \
          const T y1 = FMA(c12, da, FMA(hh, sv, x0[e]));                                                                              \
          v0[e] = w1; x0[e] = y1; a0[e] = a1[f]; j0[e] = j1[f];                                                                       \
        }                                                                                                                             \
        t0[i] = tau;                                                                                                                  \
        const int w = m_want_##SUF(a1 + 4 * (size_t)q, j1 + 4 * (size_t)q, eta2, lim, levels);                                        \
        if (w > lev[i]) lev[i] = w;                                                                                                   \
        else if (w < lev[i] && tau % (1LL << (levels - lev[i])) == 0) lev[i] -= 1;                                                    \
      }                                                                                                                               \
      ++steps;                                                                                                                        \
      evals += m;                                                                                                                     \
    }                                                                                                                                 \
    for (int i = 0; i < n && rc == 0; ++i)                                                                                            \
      if (t0[i] != end) rc = -4;                                                                                                      \
    memcpy(pos, x0, sizeof(T) * words);                                                                                               \
    memcpy(vel, v0, sizeof(T) * words);                                                                                               \
    if (substeps) *substeps = steps;                                                                                                  \
    if (row_evals) *row_evals = evals;                                                                                                \
    free(x0); free(v0); free(a0); free(j0); free(a1); free(j1); free(pts); free(pv); free(t0); free(lev); free(act);                  \
    return rc;                                                                                                                        \
  }

PASSES(float, f32, fmaf)
PASSES(double, f64, fma)
