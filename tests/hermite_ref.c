/* hermite_ref.c — an independent CPU statement of the Hermite integrator of include/nbody.h ("fourth-order Hermite integrator"), built on
 * tests/jerk_ref.c's statement of the jerk pass (compiled together with it, -ffp-contract=off: products are fused only where fmaf / fma
 * says so).  T = the precision of the words:
 *   evaluate   (a, j) of every row at (r, v): the rows form of the jerk — query i is (r_i, v_i) with skip = i, all N bodies the sources
 *   a call     (a0, j0) = evaluate(r, v); then per step, with h = dt:
 *                h2 = h * h, c2 = h2 * (T)0.5, c3 = (h2 * h) / (T)6, hh = h * (T)0.5, c12 = h2 / (T)12
 *                xp = fma(c3, j0, fma(c2, a0, fma(h, v0, x0))), vp = fma(c2, j0, fma(h, a0, v0))       per component
 *                (a1, j1) = evaluate(xp, vp)
 *                v1 = fma(c12, j0 - j1, fma(hh, a0 + a1, v0)), x1 = fma(c12, a0 - a1, fma(hh, v0 + v1, x0))
 *                the fourth value of both words is carried; (a0, j0) := (a1, j1)
 *   restarts   k calls of one step: every call evaluates (a0, j0) afresh
 *   min        per row in binary64 from the T values a2 = (ax*ax + ay*ay) + az*az, j2 likewise, q = a2 / j2; the smallest q and the lowest
 *              row that reaches it, a NaN or +inf q never; none: +inf and -1
 *   adaptive   from t = 0, after the opening evaluation and after every step, in binary64: h = eta * sqrt(min q) clamped to dt_max then
 *              dt_min, h = t_end - t if t + h > t_end, dt = (T)h, one step of dt, t += (double)dt; until t >= t_end or max_steps steps.
 * ref (binary32): the reference's d2 roundings in the jerk pass.  Test infrastructure. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

void jerk_f32(const float *pos, const float *vel, int n, const float *points, const float *pvel, int m, const int *skip, int ref,
              float *accel, float *jerk);
void jerk_f64(const double *pos, const double *vel, int n, const double *points, const double *pvel, int m, const int *skip,
              double *accel, double *jerk);

static void eval_f32(const float *pos, const float *vel, int n, const int *self, int ref, float *a, float *j) {
  jerk_f32(pos, vel, n, pos, vel, n, self, ref, a, j);
}
static void eval_f64(const double *pos, const double *vel, int n, const int *self, int ref, double *a, double *j) {
  (void)ref;
  jerk_f64(pos, vel, n, pos, vel, n, self, a, j);
}

#define HERMITE(T, SUF, FMA)                                                                                                          \
  typedef struct { int n, ref, k; int *self; T *a[2], *j[2], *x0, *v0; } run_##SUF;                                                   \
  static void open_##SUF(run_##SUF *s, const T *pos, const T *vel, int n, int ref) {                                                  \
    const size_t words = 4 * (size_t)n;                                                                                               \
    s->n = n; s->ref = ref; s->k = 0;                                                                                                 \
    s->self = (int *)malloc(sizeof(int) * (size_t)n);                                                                                 \
    for (int i = 0; i < n; ++i) s->self[i] = i;                                                                                       \
    for (int k = 0; k < 2; ++k) { s->a[k] = (T *)malloc(sizeof(T) * words); s->j[k] = (T *)malloc(sizeof(T) * words); }               \
    s->x0 = (T *)malloc(sizeof(T) * words); s->v0 = (T *)malloc(sizeof(T) * words);                                                   \
    eval_##SUF(pos, vel, n, s->self, ref, s->a[0], s->j[0]);                                                                          \
  }                                                                                                                                   \
  static void close_##SUF(run_##SUF *s) {                                                                                             \
    free(s->self); free(s->x0); free(s->v0);                                                                                          \
    for (int k = 0; k < 2; ++k) { free(s->a[k]); free(s->j[k]); }                                                                     \
  }                                                                                                                                   \
  static void step_##SUF(run_##SUF *s, T *pos, T *vel, T h) {                                                                         \
    const int n = s->n;                                                                                                               \
    const T h2 = h * h, c2 = h2 * (T)0.5, h3 = h2 * h, c3 = h3 / (T)6, hh = h * (T)0.5, c12 = h2 / (T)12;                             \
    const T *a0 = s->a[s->k], *j0 = s->j[s->k];                                                                                       \
    T *a1 = s->a[s->k ^ 1], *j1 = s->j[s->k ^ 1];                                                                                     \
    memcpy(s->x0, pos, sizeof(T) * 4 * (size_t)n);                                                                                    \
    memcpy(s->v0, vel, sizeof(T) * 4 * (size_t)n);                                                                                    \
    for (int i = 0; i < n; ++i)                                                                                                       \
      for (int c = 0; c < 3; ++c) {                                                                                                   \
        const size_t e = 4 * (size_t)i + c;                                                                                           \
        pos[e] = FMA(c3, j0[e], FMA(c2, a0[e], FMA(h, s->v0[e], s->x0[e])));                                                          \
        vel[e] = FMA(c2, j0[e], FMA(h, a0[e], s->v0[e]));                                                                             \
      }                                                                                                                               \
    eval_##SUF(pos, vel, n, s->self, s->ref, a1, j1);                                                                                 \
    for (int i = 0; i < n; ++i)                                                                                                       \
      for (int c = 0; c < 3; ++c) {                                                                                                   \
        const size_t e = 4 * (size_t)i + c;                                                                                           \
        const T dj = j0[e] - j1[e], sa = a0[e] + a1[e], da = a0[e] - a1[e];                                                           \
        const T v1 = FMA(c12, dj, FMA(hh, sa, s->v0[e]));                                                                             \
        const T sv = s->v0[e] + v1;                                                                                                   \
        vel[e] = v1;                                                                                                                  \
        pos[e] = FMA(c12, da, FMA(hh, sv, s->x0[e]));                                                                                 \
      }                                                                                                                               \
    s->k ^= 1;                                                                                                                        \
  }                                                                                                                                   \
  static void best_##SUF(const run_##SUF *s, double *q, int *row) {                                                                   \
    const T *a = s->a[s->k], *j = s->j[s->k];                                                                                         \
    double best = INFINITY;                                                                                                           \
    int br = -1;                                                                                                                      \
    for (int i = 0; i < s->n; ++i) {                                                                                                  \
      const double ax = (double)a[4 * i], ay = (double)a[4 * i + 1], az = (double)a[4 * i + 2];                                       \
      const double jx = (double)j[4 * i], jy = (double)j[4 * i + 1], jz = (double)j[4 * i + 2];                                       \
      const double a2 = (ax * ax + ay * ay) + az * az, j2 = (jx * jx + jy * jy) + jz * jz;                                            \
      const double qi = a2 / j2;                                                                                                      \
      if (qi < best) { best = qi; br = i; }                                                                                           \
    }                                                                                                                                 \
    *q = best; *row = br;                                                                                                             \
  }                                                                                                                                   \
  /* one call of nsteps steps of dt, in place */                                                                                     \
  void hermite_##SUF(T *pos, T *vel, int n, T dt, int nsteps, int ref) {                                                              \
    run_##SUF s;                                                                                                                      \
    open_##SUF(&s, pos, vel, n, ref);                                                                                                 \
    for (int k = 0; k < nsteps; ++k) step_##SUF(&s, pos, vel, dt);                                                                    \
    close_##SUF(&s);                                                                                                                  \
  }                                                                                                                                   \
  /* ncalls calls of one step each: ncalls restarts */                                                                               \
  void hermite_restarted_##SUF(T *pos, T *vel, int n, T dt, int ncalls, int ref) {                                                    \
    for (int k = 0; k < ncalls; ++k) hermite_##SUF(pos, vel, n, dt, 1, ref);                                                          \
  }                                                                                                                                   \
  void min_aarseth_##SUF(const T *pos, const T *vel, int n, int ref, double *q, int *row) {                                           \
    run_##SUF s;                                                                                                                      \
    open_##SUF(&s, pos, vel, n, ref);                                                                                                 \
    best_##SUF(&s, q, row);                                                                                                           \
    close_##SUF(&s);                                                                                                                  \
  }                                                                                                                                   \
  void hermite_adaptive_##SUF(T *pos, T *vel, int n, int ref, double eta, double t_end, double dt_min, double dt_max, int max_steps,  \
                              double *t_reached, int *steps_taken) {                                                                  \
    run_##SUF s;                                                                                                                      \
    double t = 0.0;                                                                                                                   \
    int steps = 0;                                                                                                                    \
    open_##SUF(&s, pos, vel, n, ref);                                                                                                 \
    while (t < t_end && steps < max_steps) {                                                                                          \
      double q, h;                                                                                                                    \
      int row;                                                                                                                        \
      best_##SUF(&s, &q, &row);                                                                                                       \
      h = eta * sqrt(q);                                                                                                              \
      if (h > dt_max) h = dt_max;                                                                                                     \
      if (h < dt_min) h = dt_min;                                                                                                     \
      if (t + h > t_end) h = t_end - t;                                                                                               \
      const T dt = (T)h;                                                                                                              \
      step_##SUF(&s, pos, vel, dt);                                                                                                   \
      t += (double)dt;                                                                                                                \
      ++steps;                                                                                                                        \
    }                                                                                                                                 \
    *t_reached = t; *steps_taken = steps;                                                                                             \
    close_##SUF(&s);                                                                                                                  \
  }

HERMITE(float, f32, fmaf)
HERMITE(double, f64, fma)
