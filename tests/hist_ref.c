/* hist_ref.c — an independent CPU statement of include/nbody.h ("radial counts, pair histogram"): per query one ascending scan over
 * the bodies,
 *   dx = xj - x, dy = yj - y, dz = zj - z;  d2 = fma(dx, dx, fma(dy, dy, dz * dz))      (no softening; the context precision)
 * that leaves the excluded body out and keeps the cumulative counts c_b = #{ j : d2_j < edges2[b] }; counts[b] = c_(b+1) - c_b.  A NaN
 * d2 is below nothing, nor is a +inf d2 below a +inf edge.  The pair histogram is a scan of its own over i < j — not half of the rows
 * form — so the two statements check each other.  Test infrastructure, compiled by the hist tests with -ffp-contract=off (products
 * are fused only where fmaf / fma says so); queries are independent, so an OpenMP build changes nothing. */
#include <math.h>
#include <stddef.h>

#define HIST_MAX_BINS 32

/* pos: n words of 4 floats.  points: m words of 4 floats, or NULL: the rows form, query p is body first + p and leaves itself out.
 * skip (points form): NULL or m ints (-1: none).  edges2: n_bins + 1 values, non-decreasing.  counts: m x n_bins ints, bin b of query p
 * at p * n_bins + b.  1 <= n_bins <= HIST_MAX_BINS. */
void hist_f32(const float *pos, int n, const float *points, int first, int m, const int *skip, const float *edges2, int n_bins, int *counts) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const float *q = points ? points + 4 * (size_t)p : pos + 4 * (size_t)(first + p);
    const float x = q[0], y = q[1], z = q[2];
    const int sk = points ? (skip ? skip[p] : -1) : first + p;
    int cum[HIST_MAX_BINS + 1];
    for (int b = 0; b <= n_bins; ++b) cum[b] = 0;
    for (int j = 0; j < n; ++j) {
      if (j == sk) continue;
      const float dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const float v = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      for (int b = 0; b <= n_bins; ++b) cum[b] += v < edges2[b];
    }
    for (int b = 0; b < n_bins; ++b) counts[(size_t)p * n_bins + b] = cum[b + 1] - cum[b];
  }
}

/* the unordered pairs i < j of the whole system by a scan of their own (d2 from i's side), the same cumulative rule, 64-bit */
void pair_hist_f32(const float *pos, int n, const float *edges2, int n_bins, long long *pairs) {
  long long cum[HIST_MAX_BINS + 1];
  for (int b = 0; b <= n_bins; ++b) cum[b] = 0;
  for (int i = 0; i < n; ++i) {
    const float x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    for (int j = i + 1; j < n; ++j) {
      const float dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const float v = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      for (int b = 0; b <= n_bins; ++b) cum[b] += v < edges2[b];
    }
  }
  for (int b = 0; b < n_bins; ++b) pairs[b] = cum[b + 1] - cum[b];
}

/* pos: n words of 4 doubles.  points: m words of 4 doubles, or NULL: the rows form, query p is body first + p and leaves itself out.
 * skip (points form): NULL or m ints (-1: none).  edges2: n_bins + 1 values, non-decreasing.  counts: m x n_bins ints, bin b of query p
 * at p * n_bins + b.  1 <= n_bins <= HIST_MAX_BINS. */
void hist_f64(const double *pos, int n, const double *points, int first, int m, const int *skip, const double *edges2, int n_bins, int *counts) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const double *q = points ? points + 4 * (size_t)p : pos + 4 * (size_t)(first + p);
    const double x = q[0], y = q[1], z = q[2];
    const int sk = points ? (skip ? skip[p] : -1) : first + p;
    int cum[HIST_MAX_BINS + 1];
    for (int b = 0; b <= n_bins; ++b) cum[b] = 0;
    for (int j = 0; j < n; ++j) {
      if (j == sk) continue;
      const double dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const double v = fma(dx, dx, fma(dy, dy, dz * dz));
      for (int b = 0; b <= n_bins; ++b) cum[b] += v < edges2[b];
    }
    for (int b = 0; b < n_bins; ++b) counts[(size_t)p * n_bins + b] = cum[b + 1] - cum[b];
  }
}

/* the unordered pairs i < j of the whole system by a scan of their own (d2 from i's side), the same cumulative rule, 64-bit */
void pair_hist_f64(const double *pos, int n, const double *edges2, int n_bins, long long *pairs) {
  long long cum[HIST_MAX_BINS + 1];
  for (int b = 0; b <= n_bins; ++b) cum[b] = 0;
  for (int i = 0; i < n; ++i) {
    const double x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    for (int j = i + 1; j < n; ++j) {
      const double dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const double v = fma(dx, dx, fma(dy, dy, dz * dz));
      for (int b = 0; b <= n_bins; ++b) cum[b] += v < edges2[b];
    }
  }
  for (int b = 0; b < n_bins; ++b) pairs[b] = cum[b + 1] - cum[b];
}
