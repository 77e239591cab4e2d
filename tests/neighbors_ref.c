/* neighbors_ref.c — an independent CPU statement of include/nbody.h ("nearest neighbour, radius count, closest pair"): per query one
 * ascending scan over the bodies,
 *   dx = xj - x, dy = yj - y, dz = zj - z;  d2 = fma(dx, dx, fma(dy, dy, dz * dz))      (no softening; the context precision)
 * from (best = +inf, idx = -1, count = 0), the excluded body left out, replacing on strict < (so the lowest j wins a tie and neither a
 * NaN nor a +inf d2 is ever chosen) and counting d2 <= r2 (NaN never counts).  The closest pair is a scan of its own over all i < j
 * in ascending (i, j) with strict <, not a reduction of the rows.  Test infrastructure, compiled by the neighbour tests with
 * -ffp-contract=off (products are fused only where fmaf / fma says so); queries are independent, so an OpenMP build changes nothing. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

/* pos: n words of 4 floats.  points: m words of 4 floats, or NULL: the rows form, query p is body first + p and leaves itself out.
 * skip (points form): NULL or m ints (-1: none).  idx, d2: m values.  count: m values or NULL (r2 is then ignored). */
void neighbors_f32(const float *pos, int n, const float *points, int first, int m, const int *skip, float r2, int *idx, float *d2,
                   int *count) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const float *q = points ? points + 4 * (size_t)p : pos + 4 * (size_t)(first + p);
    const float x = q[0], y = q[1], z = q[2];
    const int sk = points ? (skip ? skip[p] : -1) : first + p;
    float best = INFINITY;
    int bi = -1, c = 0;
    for (int j = 0; j < n; ++j) {
      if (j == sk) continue;
      const float dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const float v = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      if (v < best) { best = v; bi = j; }
      if (count && v <= r2) ++c;
    }
    idx[p] = bi;
    d2[p] = best;
    if (count) count[p] = c;
  }
}

/* the same with words of 4 doubles */
void neighbors_f64(const double *pos, int n, const double *points, int first, int m, const int *skip, double r2, int *idx, double *d2,
                   int *count) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const double *q = points ? points + 4 * (size_t)p : pos + 4 * (size_t)(first + p);
    const double x = q[0], y = q[1], z = q[2];
    const int sk = points ? (skip ? skip[p] : -1) : first + p;
    double best = INFINITY;
    int bi = -1, c = 0;
    for (int j = 0; j < n; ++j) {
      if (j == sk) continue;
      const double dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const double v = fma(dx, dx, fma(dy, dy, dz * dz));
      if (v < best) { best = v; bi = j; }
      if (count && v <= r2) ++c;
    }
    idx[p] = bi;
    d2[p] = best;
    if (count) count[p] = c;
  }
}

/* out[0] < out[1] of the smallest d2 over all pairs, ties to the lowest i, then the lowest j (-1, -1, +inf without a pair): per i the
 * best j > i in ascending j with strict <, then the rows' bests in ascending i with strict < */
void closest_pair_f32(const float *pos, int n, int *out, float *d2) {
  float *bd = (float *)malloc((size_t)n * sizeof(float));
  int *bj = (int *)malloc((size_t)n * sizeof(int));
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; ++i) {
    const float x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    bd[i] = INFINITY;
    bj[i] = -1;
    for (int j = i + 1; j < n; ++j) {
      const float dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const float v = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      if (v < bd[i]) { bd[i] = v; bj[i] = j; }
    }
  }
  out[0] = out[1] = -1;
  *d2 = INFINITY;
  for (int i = 0; i < n; ++i)
    if (bd[i] < *d2) { *d2 = bd[i]; out[0] = i; out[1] = bj[i]; }
  free(bd);
  free(bj);
}

void closest_pair_f64(const double *pos, int n, int *out, double *d2) {
  double *bd = (double *)malloc((size_t)n * sizeof(double));
  int *bj = (int *)malloc((size_t)n * sizeof(int));
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; ++i) {
    const double x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    bd[i] = INFINITY;
    bj[i] = -1;
    for (int j = i + 1; j < n; ++j) {
      const double dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const double v = fma(dx, dx, fma(dy, dy, dz * dz));
      if (v < bd[i]) { bd[i] = v; bj[i] = j; }
    }
  }
  out[0] = out[1] = -1;
  *d2 = INFINITY;
  for (int i = 0; i < n; ++i)
    if (bd[i] < *d2) { *d2 = bd[i]; out[0] = i; out[1] = bj[i]; }
  free(bd);
  free(bj);
}
