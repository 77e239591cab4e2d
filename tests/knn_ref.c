/* knn_ref.c — an independent CPU statement of include/nbody.h ("k nearest neighbours"): per query one ascending scan over the bodies,
 *   dx = xj - x, dy = yj - y, dz = zj - z;  d2 = fma(dx, dx, fma(dy, dy, dz * dz))      (no softening; the context precision)
 * that starts from k entries (d2 = +inf, idx = -1), leaves the excluded body out, puts a candidate behind every entry with d2 <= its
 * own and drops the last entry.  A candidate has d2 < +inf: a d2 that is not below the list's last entry — a NaN, a +inf, or one that
 * is too large — changes nothing, and since the last entry is never above +inf this is the same rule.  Test infrastructure, compiled
 * by the knn tests with -ffp-contract=off (products are fused only where fmaf / fma says so); queries are independent, so an OpenMP
 * build changes nothing. */
#include <math.h>
#include <stddef.h>

#define KNN_MAX 32

/* pos: n words of 4 floats.  points: m words of 4 floats, or NULL: the rows form, query p is body first + p and leaves itself out.
 * skip (points form): NULL or m ints (-1: none).  idx, d2: m x k values, entry r of query p at p * k + r.  1 <= k <= KNN_MAX. */
void knn_f32(const float *pos, int n, const float *points, int first, int m, const int *skip, int k, int *idx, float *d2) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const float *q = points ? points + 4 * (size_t)p : pos + 4 * (size_t)(first + p);
    const float x = q[0], y = q[1], z = q[2];
    const int sk = points ? (skip ? skip[p] : -1) : first + p;
    float ld[KNN_MAX];
    int li[KNN_MAX];
    for (int r = 0; r < k; ++r) { ld[r] = INFINITY; li[r] = -1; }
    for (int j = 0; j < n; ++j) {
      if (j == sk) continue;
      const float dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const float v = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      if (!(v < ld[k - 1])) continue;
      int r = k - 1;   /* behind every entry with d2 <= v: entries above v move one place down, the last one out */
      for (; r > 0 && v < ld[r - 1]; --r) { ld[r] = ld[r - 1]; li[r] = li[r - 1]; }
      ld[r] = v;
      li[r] = j;
    }
    for (int r = 0; r < k; ++r) { idx[(size_t)p * k + r] = li[r]; d2[(size_t)p * k + r] = ld[r]; }
  }
}

/* the same with words of 4 doubles */
void knn_f64(const double *pos, int n, const double *points, int first, int m, const int *skip, int k, int *idx, double *d2) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const double *q = points ? points + 4 * (size_t)p : pos + 4 * (size_t)(first + p);
    const double x = q[0], y = q[1], z = q[2];
    const int sk = points ? (skip ? skip[p] : -1) : first + p;
    double ld[KNN_MAX];
    int li[KNN_MAX];
    for (int r = 0; r < k; ++r) { ld[r] = INFINITY; li[r] = -1; }
    for (int j = 0; j < n; ++j) {
      if (j == sk) continue;
      const double dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const double v = fma(dx, dx, fma(dy, dy, dz * dz));
      if (!(v < ld[k - 1])) continue;
      int r = k - 1;
      for (; r > 0 && v < ld[r - 1]; --r) { ld[r] = ld[r - 1]; li[r] = li[r - 1]; }
      ld[r] = v;
      li[r] = j;
    }
    for (int r = 0; r < k; ++r) { idx[(size_t)p * k + r] = li[r]; d2[(size_t)p * k + r] = ld[r]; }
  }
}
