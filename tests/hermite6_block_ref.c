/* hermite6_block_ref.c — an independent CPU statement of the sixth-order Hermite integrator's individual block time steps of
 * include/nbody.h ("sixth-order individual block time steps"), built on tests/snap_ref.c's statement of the snap at points with a skip
 * index (compiled together with it, -ffp-contract=off: products are fused only where fmaf / fma says so).  T = the precision of the words:
 *   time      integer ticks of unit = (T)(dt_max * 2^-(levels - 1)); row i carries t0_i, k_i and its base (x0, v0, a0, j0, s0, c0); its
 *             step is s_i = 2^(levels - 1 - k_i) ticks
 *   want      hermite_block_ref.c's, from (a, j) alone: in binary64 from the T values a2 = (ax*ax + ay*ay) + az*az, j2 likewise,
 *             q = a2 / j2; q not < +inf: 0; else e = eta2 * q with eta2 = (double)eta * (double)eta, lim[k] = (d 2^-k)^2 with
 *             d = (double)dt_max: the smallest k with lim[k] <= e, else levels - 1
 *   start     base := the state, (a0, j0, s0) := snap_rows (the two passes of nbody_snap_rows), c0 := +0, t0 := 0, k := want
 *   sub-step  tau := min (t0_i + s_i); every row predicted from its base with h_i = (T)(tau - t0_i) * unit and the coefficients of h_i
 *             (hermite6_ref.c's expressions: xp, vp, ap); the rows with t0_i + s_i = tau, ascending, are evaluated by the snap at
 *             points — query (xp_i, vp_i, ap_i), skip = i, sources the predicted (xp, vp, ap) of all rows — and corrected with their own
 *             h_i (v1, x1 and the crackle c1 with r = 1 / h_i); base := (x1, v1, a1, j1, s1, c1), t0 := tau; w = want(a1, j1): w > k:
 *             k := w; w < k and tau mod 2^(levels - k) == 0: k := k - 1
 *   end       tau = nblocks * 2^(levels - 1); the state is the base of every row (all at that time: asserted, as is the invariant that
 *             every t0_i is a multiple of s_i — a violation returns a negative value)
 * The trace, where asked for, is hermite_block_ref.c's: level0[n] the first levels; per sub-step tau and the active count; the active
 * rows of all sub-steps one after another with the level each goes on with.  flags: bit 0 ref (binary32: the reference's d2 roundings),
 * bit 1 mass (the sources weigh the w of their position word).  Test infrastructure. */
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

#define BLOCK6(T, SUF, FMA)                                                                                                           \
  static int want6_##SUF(const T *a, const T *j, double eta2, const double *lim, int levels) {                                        \
    const double ax = (double)a[0], ay = (double)a[1], az = (double)a[2], jx = (double)j[0], jy = (double)j[1], jz = (double)j[2];    \
    const double a2 = (ax * ax + ay * ay) + az * az, j2 = (jx * jx + jy * jy) + jz * jz;                                              \
    const double q = a2 / j2;                                                                                                         \
    if (!(q < INFINITY)) return 0;                                                                                                    \
    const double e = eta2 * q;                                                                                                        \
    for (int k = 0; k < levels; ++k)                                                                                                  \
      if (lim[k] <= e) return k;                                                                                                      \
    return levels - 1;                                                                                                                \
  }                                                                                                                                   \
  /* in place; returns 0, or a negative value where the invariant or a trace capacity fails */                                       \
  int hermite6_block_##SUF(T *pos, T *vel, int n, int flags, T eta, T dt_max, int levels, int nblocks, long long *substeps,           \
                           long long *row_evals, long long *tr_tau, int *tr_count, int *tr_rows, int *tr_levels, int *tr_level0,      \
                           long long cap_steps, long long cap_rows) {                                                                 \
    const int ref = flags & 1, mass = (flags >> 1) & 1;                                                                               \
    const size_t words = 4 * (size_t)n;                                                                                               \
    const T unit = (T)ldexp((double)dt_max, -(levels - 1));                                                                           \
    const double eta2 = (double)eta * (double)eta;                                                                                    \
    double lim[64];                                                                                                                   \
    for (int k = 0; k < levels; ++k) { const double dk = ldexp((double)dt_max, -k); lim[k] = dk * dk; }                               \
    T *buf = (T *)calloc(13 * words, sizeof(T));                                                                                      \
    T *x0 = buf, *v0 = buf + words, *a0 = buf + 2 * words, *j0 = buf + 3 * words, *s0 = buf + 4 * words, *c0 = buf + 5 * words;       \
    T *ap = buf + 6 * words, *a1 = buf + 7 * words, *j1 = buf + 8 * words, *s1 = buf + 9 * words;                                     \
    T *pts = buf + 10 * words, *pv = buf + 11 * words, *pa = buf + 12 * words;                                                        \
    long long *t0 = (long long *)calloc((size_t)n, sizeof(long long));                                                                \
    int *lev = (int *)malloc(sizeof(int) * (size_t)n), *act = (int *)malloc(sizeof(int) * (size_t)n);                                 \
    const long long end = (long long)nblocks << (levels - 1);                                                                         \
    long long steps = 0, evals = 0, tau = 0;                                                                                          \
    int rc = 0;                                                                                                                       \
    memcpy(x0, pos, sizeof(T) * words);                                                                                               \
    memcpy(v0, vel, sizeof(T) * words);                                                                                               \
    snap_rows_##SUF(pos, vel, n, ref, mass, a0, j0, s0);                                                                              \
    for (int i = 0; i < n; ++i) {                                                                                                     \
      lev[i] = want6_##SUF(a0 + 4 * (size_t)i, j0 + 4 * (size_t)i, eta2, lim, levels);                                                \
      if (tr_level0) tr_level0[i] = lev[i];                                                                                           \
    }                                                                                                                                 \
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
        const T h2 = h * h, c2 = h2 * (T)0.5, h3 = h2 * h, c3 = h3 / (T)6, h4 = h2 * h2, c4 = h4 / (T)24, h5 = h4 * h, c5 = h5 / (T)120; \
        for (int c = 0; c < 3; ++c) {                                                                                                 \
          const size_t e = 4 * (size_t)i + c;                                                                                         \
          pos[e] = FMA(c5, c0[e], FMA(c4, s0[e], FMA(c3, j0[e], FMA(c2, a0[e], FMA(h, v0[e], x0[e])))));                              \
          vel[e] = FMA(c4, c0[e], FMA(c3, s0[e], FMA(c2, j0[e], FMA(h, a0[e], v0[e]))));                                              \
          ap[e] = FMA(c3, c0[e], FMA(c2, s0[e], FMA(h, j0[e], a0[e])));                                                               \
        }                                                                                                                             \
        pos[4 * (size_t)i + 3] = x0[4 * (size_t)i + 3];                                                                               \
        vel[4 * (size_t)i + 3] = v0[4 * (size_t)i + 3];                                                                               \
      }                                                                                                                               \
      for (int q = 0; q < m; ++q) {                                                                                                   \
        memcpy(pts + 4 * (size_t)q, pos + 4 * (size_t)act[q], sizeof(T) * 4);                                                         \
        memcpy(pv + 4 * (size_t)q, vel + 4 * (size_t)act[q], sizeof(T) * 4);                                                          \
        memcpy(pa + 4 * (size_t)q, ap + 4 * (size_t)act[q], sizeof(T) * 4);                                                           \
      }                                                                                                                               \
      snap_##SUF(pos, vel, ap, n, pts, pv, pa, m, act, ref, mass, a1, j1, s1);                                                        \
      if (tr_tau && (steps >= cap_steps || evals + m > cap_rows)) { rc = -3; break; }                                                 \
      if (tr_tau) { tr_tau[steps] = tau; tr_count[steps] = m; }                                                                       \
      for (int q = 0; q < m; ++q) {                                                                                                   \
        const int i = act[q];                                                                                                         \
        const T h = (T)(tau - t0[i]) * unit;                                                                                          \
        const T h2 = h * h, h3 = h2 * h, hh = h * (T)0.5, c10 = h2 / (T)10, c120 = h3 / (T)120, r = (T)1 / h;                         \
        for (int c = 0; c < 3; ++c) {                                                                                                 \
          const size_t e = 4 * (size_t)i + c, f = 4 * (size_t)q + c;                                                                  \
          const T ss = s0[e] + s1[f], dj = j0[e] - j1[f], sa = a0[e] + a1[f], sj = j0[e] + j1[f], da = a0[e] - a1[f];                 \
          const T w1 = FMA(c120, ss, FMA(c10, dj, FMA(hh, sa, v0[e])));                                                               \
          const T sv = v0[e] + w1;                                                                                                    \
          const T y1 = FMA(c120, sj, FMA(c10, da, FMA(hh, sv, x0[e])));                                                               \
          const T d1 = a1[f] - a0[e];                                                                                                 \
          const T e1 = (T)60 * d1;                                                                                                    \
          const T p24 = (T)24 * j0[e];                                                                                                \
          const T e2 = FMA((T)36, j1[f], p24);                                                                                        \
          const T m3 = (T)-3 * s0[e];                                                                                                 \
          const T e3 = FMA((T)9, s1[f], m3);                                                                                          \
          const T in = FMA(r, FMA(r, e1, -e2), e3);                                                                                   \
          v0[e] = w1; x0[e] = y1; a0[e] = a1[f]; j0[e] = j1[f]; s0[e] = s1[f]; c0[e] = r * in;                                        \
          pos[e] = y1; vel[e] = w1;                                                                                                   \
        }                                                                                                                             \
        t0[i] = tau;                                                                                                                  \
        const int w = want6_##SUF(a1 + 4 * (size_t)q, j1 + 4 * (size_t)q, eta2, lim, levels);                                         \
        if (w > lev[i]) lev[i] = w;                                                                                                   \
        else if (w < lev[i] && tau % (1LL << (levels - lev[i])) == 0) lev[i] -= 1;                                                    \
        if (tr_tau) { tr_rows[evals + q] = i; tr_levels[evals + q] = lev[i]; }                                                        \
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
    free(buf); free(t0); free(lev); free(act);                                                                                        \
    return rc;                                                                                                                        \
  }

BLOCK6(float, f32, fmaf)
BLOCK6(double, f64, fma)
