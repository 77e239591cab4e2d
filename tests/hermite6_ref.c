/* hermite6_ref.c — an independent CPU statement of the sixth-order Hermite integrator of include/nbody.h ("sixth-order Hermite
 * integrator"; Nitadori & Makino 2008), built on tests/snap_ref.c's statement of the snap pass (compiled together with it,
 * -ffp-contract=off: products are fused only where fmaf / fma says so).  T = the precision of the words:
 *   a call     (a0, j0, s0) = snap_rows(r, v) — the two passes of nbody_snap_rows —, c0 = +0; then per step, with h = dt:
 *                h2 = h * h, c2 = h2 * (T)0.5, c3 = (h2 * h) / (T)6, c4 = (h2 * h2) / (T)24, c5 = ((h2 * h2) * h) / (T)120,
 *                hh = h * (T)0.5, c10 = h2 / (T)10, c120 = (h2 * h) / (T)120, r = (T)1 / h
 *                xp = fma(c5, c0, fma(c4, s0, fma(c3, j0, fma(c2, a0, fma(h, v0, x0)))))
 *                vp = fma(c4, c0, fma(c3, s0, fma(c2, j0, fma(h, a0, v0))))
 *                ap = fma(c3, c0, fma(c2, s0, fma(h, j0, a0)))                                        per component
 *                (a1, j1, s1) = the snap pass with sources (xp, vp, ap), row i's query (xp_i, vp_i, ap_i), skip = i
 *                v1 = fma(c120, s0 + s1, fma(c10, j0 - j1, fma(hh, a0 + a1, v0)))
 *                x1 = fma(c120, j0 + j1, fma(c10, a0 - a1, fma(hh, v0 + v1, x0)))
 *                e1 = 60 * (a1 - a0), e2 = fma(36, j1, 24 * j0), e3 = fma(9, s1, -3 * s0), c1 = r * fma(r, fma(r, e1, -e2), e3)
 *                the fourth value of both words is carried; (a0, j0, s0, c0) := (a1, j1, s1, c1)
 *              crackle = 0 (a test's wrong scheme, never the library's): c1 is left at +0, the fifth-order scheme the order test tells apart
 *   restarts   k calls of one step: every call evaluates (a0, j0, s0) afresh and starts from c0 = +0
 *   adaptive   hermite_ref.c's loop over these steps: q = min |a|^2 / |j|^2 in binary64 from the carried T values.
 * ref (binary32): the reference's d2 roundings; mass: the sources weigh the w of their position word.  Test infrastructure. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#define DECLARE(T, SUF)                                                                                                                 \
  void snap_##SUF(const T *pos, const T *vel, const T *acc, int n, const T *points, const T *pvel, const T *pacc, int m,               \
                  const int *skip, int ref, int mass, T *accel, T *jerk, T *snap);                                                     \
  void snap_rows_##SUF(const T *pos, const T *vel, int n, int ref, int mass, T *accel, T *jerk, T *snap);
DECLARE(float, f32)
DECLARE(double, f64)

#define HERMITE6(T, SUF, FMA)                                                                                                           \
  typedef struct { int n, ref, mass, crackle, k; int *self; T *a[2], *j[2], *s[2], *c, *ap, *x0, *v0; } run6_##SUF;                     \
  static void open6_##SUF(run6_##SUF *s, const T *pos, const T *vel, int n, int ref, int mass, int crackle) {                           \
    const size_t words = 4 * (size_t)n;                                                                                                 \
    s->n = n; s->ref = ref; s->mass = mass; s->crackle = crackle; s->k = 0;                                                             \
    s->self = (int *)malloc(sizeof(int) * (size_t)n);                                                                                   \
    for (int i = 0; i < n; ++i) s->self[i] = i;                                                                                         \
    for (int k = 0; k < 2; ++k) {                                                                                                       \
      s->a[k] = (T *)malloc(sizeof(T) * words); s->j[k] = (T *)malloc(sizeof(T) * words); s->s[k] = (T *)malloc(sizeof(T) * words);     \
    }                                                                                                                                   \
    s->c = (T *)calloc(words, sizeof(T)); s->ap = (T *)calloc(words, sizeof(T));                                                        \
    s->x0 = (T *)malloc(sizeof(T) * words); s->v0 = (T *)malloc(sizeof(T) * words);                                                     \
    snap_rows_##SUF(pos, vel, n, ref, mass, s->a[0], s->j[0], s->s[0]);                                                                 \
  }                                                                                                                                     \
  static void close6_##SUF(run6_##SUF *s) {                                                                                             \
    free(s->self); free(s->c); free(s->ap); free(s->x0); free(s->v0);                                                                   \
    for (int k = 0; k < 2; ++k) { free(s->a[k]); free(s->j[k]); free(s->s[k]); }                                                        \
  }                                                                                                                                     \
  static void step6_##SUF(run6_##SUF *s, T *pos, T *vel, T h) {                                                                         \
    const int n = s->n;                                                                                                                 \
    const T h2 = h * h, c2 = h2 * (T)0.5, h3 = h2 * h, c3 = h3 / (T)6, h4 = h2 * h2, c4 = h4 / (T)24, h5 = h4 * h, c5 = h5 / (T)120;    \
    const T hh = h * (T)0.5, c10 = h2 / (T)10, c120 = h3 / (T)120, r = (T)1 / h;                                                        \
    const T *a0 = s->a[s->k], *j0 = s->j[s->k], *s0 = s->s[s->k];                                                                       \
    T *a1 = s->a[s->k ^ 1], *j1 = s->j[s->k ^ 1], *s1 = s->s[s->k ^ 1], *c0 = s->c;                                                     \
    memcpy(s->x0, pos, sizeof(T) * 4 * (size_t)n);                                                                                      \
    memcpy(s->v0, vel, sizeof(T) * 4 * (size_t)n);                                                                                      \
    for (int i = 0; i < n; ++i)                                                                                                         \
      for (int c = 0; c < 3; ++c) {                                                                                                     \
        const size_t e = 4 * (size_t)i + c;                                                                                             \
        pos[e] = FMA(c5, c0[e], FMA(c4, s0[e], FMA(c3, j0[e], FMA(c2, a0[e], FMA(h, s->v0[e], s->x0[e])))));                            \
        vel[e] = FMA(c4, c0[e], FMA(c3, s0[e], FMA(c2, j0[e], FMA(h, a0[e], s->v0[e]))));                                               \
        s->ap[e] = FMA(c3, c0[e], FMA(c2, s0[e], FMA(h, j0[e], a0[e])));                                                                \
      }                                                                                                                                 \
    snap_##SUF(pos, vel, s->ap, n, pos, vel, s->ap, n, s->self, s->ref, s->mass, a1, j1, s1);                                           \
    for (int i = 0; i < n; ++i)                                                                                                         \
      for (int c = 0; c < 3; ++c) {                                                                                                     \
        const size_t e = 4 * (size_t)i + c;                                                                                             \
        const T ss = s0[e] + s1[e], dj = j0[e] - j1[e], sa = a0[e] + a1[e], sj = j0[e] + j1[e], da = a0[e] - a1[e];                     \
        const T v1 = FMA(c120, ss, FMA(c10, dj, FMA(hh, sa, s->v0[e])));                                                                \
        const T sv = s->v0[e] + v1;                                                                                                     \
        vel[e] = v1;                                                                                                                    \
        pos[e] = FMA(c120, sj, FMA(c10, da, FMA(hh, sv, s->x0[e])));                                                                    \
        const T d1 = a1[e] - a0[e];                                                                                                     \
        const T e1 = (T)60 * d1;                                                                                                        \
        const T p24 = (T)24 * j0[e];                                                                                                    \
        const T e2 = FMA((T)36, j1[e], p24);                                                                                            \
        const T m3 = (T)-3 * s0[e];                                                                                                     \
        const T e3 = FMA((T)9, s1[e], m3);                                                                                              \
        const T in = FMA(r, FMA(r, e1, -e2), e3);                                                                                       \
        if (s->crackle) c0[e] = r * in;                                                                                                 \
      }                                                                                                                                 \
    s->k ^= 1;                                                                                                                          \
  }                                                                                                                                     \
  static void best6_##SUF(const run6_##SUF *s, double *q, int *row) {                                                                   \
    const T *a = s->a[s->k], *j = s->j[s->k];                                                                                           \
    double best = INFINITY;                                                                                                             \
    int br = -1;                                                                                                                        \
    for (int i = 0; i < s->n; ++i) {                                                                                                    \
      const double ax = (double)a[4 * i], ay = (double)a[4 * i + 1], az = (double)a[4 * i + 2];                                         \
      const double jx = (double)j[4 * i], jy = (double)j[4 * i + 1], jz = (double)j[4 * i + 2];                                         \
      const double a2 = (ax * ax + ay * ay) + az * az, j2 = (jx * jx + jy * jy) + jz * jz;                                              \
      const double qi = a2 / j2;                                                                                                        \
      if (qi < best) { best = qi; br = i; }                                                                                             \
    }                                                                                                                                   \
    *q = best; *row = br;                                                                                                               \
  }                                                                                                                                     \
  /* one call of nsteps steps of dt, in place.  flags: bit 0 ref, bit 1 mass, bit 2 NO crackle (the wrong scheme) */                   \
  void hermite6_##SUF(T *pos, T *vel, int n, T dt, int nsteps, int flags) {                                                             \
    run6_##SUF s;                                                                                                                       \
    open6_##SUF(&s, pos, vel, n, flags & 1, (flags >> 1) & 1, !(flags & 4));                                                            \
    for (int k = 0; k < nsteps; ++k) step6_##SUF(&s, pos, vel, dt);                                                                     \
    close6_##SUF(&s);                                                                                                                   \
  }                                                                                                                                     \
  /* ncalls calls of one step each: ncalls restarts */                                                                                 \
  void hermite6_restarted_##SUF(T *pos, T *vel, int n, T dt, int ncalls, int flags) {                                                   \
    for (int k = 0; k < ncalls; ++k) hermite6_##SUF(pos, vel, n, dt, 1, flags);                                                         \
  }                                                                                                                                     \
  void hermite6_adaptive_##SUF(T *pos, T *vel, int n, int flags, double eta, double t_end, double dt_min, double dt_max, int max_steps, \
                               double *t_reached, int *steps_taken) {                                                                   \
    run6_##SUF s;                                                                                                                       \
    double t = 0.0;                                                                                                                     \
    int steps = 0;                                                                                                                      \
    open6_##SUF(&s, pos, vel, n, flags & 1, (flags >> 1) & 1, !(flags & 4));                                                            \
    while (t < t_end && steps < max_steps) {                                                                                            \
      double q, h;                                                                                                                      \
      int row;                                                                                                                          \
      best6_##SUF(&s, &q, &row);                                                                                                        \
      h = eta * sqrt(q);                                                                                                                \
      if (h > dt_max) h = dt_max;                                                                                                       \
      if (h < dt_min) h = dt_min;                                                                                                       \
      if (t + h > t_end) h = t_end - t;                                                                                                 \
      const T dt = (T)h;                                                                                                                \
      step6_##SUF(&s, pos, vel, dt);                                                                                                    \
      t += (double)dt;                                                                                                                  \
      ++steps;                                                                                                                          \
    }                                                                                                                                   \
    *t_reached = t; *steps_taken = steps;                                                                                               \
    close6_##SUF(&s);                                                                                                                   \
  }

HERMITE6(float, f32, fmaf)
HERMITE6(double, f64, fma)
