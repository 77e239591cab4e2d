/* timescale_ref.c — an independent CPU statement of include/nbody.h ("pair time scales and a shared adaptive time step"): per row i one
 * ascending scan over the bodies j != i,
 *   dx = xj - xi, dy = yj - yi, dz = zj - zi;        d2 = fma(dx, dx, fma(dy, dy, dz * dz))      (no softening; the context precision)
 *   ux = vxj - vxi, uy = vyj - vyi, uz = vzj - vzi;  v2 = fma(ux, ux, fma(uy, uy, uz * uz))
 *   q = d2 / v2
 * from (tau2 = +inf, idx = -1, d2min = +inf), replacing on strict < (so the lowest j wins a tie and neither a NaN nor a +inf is ever
 * chosen).  The system form is a scan of its own over the rows in ascending i with strict <.  Test infrastructure, compiled by the
 * time-scale tests with -ffp-contract=off (products are fused only where fmaf / fma says so); rows are independent, so an OpenMP build
 * changes nothing. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

/* pos, vel: n words of 4 floats.  Rows first .. first + m - 1.  tau2, idx, d2min: m values each. */
void timescale_f32(const float *pos, const float *vel, int n, int first, int m, float *tau2, int *idx, float *d2min) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const int i = first + p;
    const float x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    const float vx = vel[4 * (size_t)i], vy = vel[4 * (size_t)i + 1], vz = vel[4 * (size_t)i + 2];
    float best = INFINITY, dmin = INFINITY;
    int bi = -1;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const float dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const float ux = vel[4 * (size_t)j] - vx, uy = vel[4 * (size_t)j + 1] - vy, uz = vel[4 * (size_t)j + 2] - vz;
      const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      const float v2 = fmaf(ux, ux, fmaf(uy, uy, uz * uz));
      const float q = d2 / v2;
      if (q < best) { best = q; bi = j; }
      if (d2 < dmin) dmin = d2;
    }
    tau2[p] = best;
    idx[p] = bi;
    d2min[p] = dmin;
  }
}

/* the same with words of 4 doubles */
void timescale_f64(const double *pos, const double *vel, int n, int first, int m, double *tau2, int *idx, double *d2min) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const int i = first + p;
    const double x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    const double vx = vel[4 * (size_t)i], vy = vel[4 * (size_t)i + 1], vz = vel[4 * (size_t)i + 2];
    double best = INFINITY, dmin = INFINITY;
    int bi = -1;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const double dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const double ux = vel[4 * (size_t)j] - vx, uy = vel[4 * (size_t)j + 1] - vy, uz = vel[4 * (size_t)j + 2] - vz;
      const double d2 = fma(dx, dx, fma(dy, dy, dz * dz));
      const double v2 = fma(ux, ux, fma(uy, uy, uz * uz));
      const double q = d2 / v2;
      if (q < best) { best = q; bi = j; }
      if (d2 < dmin) dmin = d2;
    }
    tau2[p] = best;
    idx[p] = bi;
    d2min[p] = dmin;
  }
}

/* the whole system: out[0] = the lowest row that reaches the smallest tau2, out[1] = its partner (-1, -1 and +inf without one), and
 * the smallest d2min: the rows in ascending i with strict < */
void min_timescale_f32(const float *pos, const float *vel, int n, float *tau2, int *out, float *d2min) {
  float *t = (float *)malloc((size_t)n * sizeof(float)), *d = (float *)malloc((size_t)n * sizeof(float));
  int *ix = (int *)malloc((size_t)n * sizeof(int));
  timescale_f32(pos, vel, n, 0, n, t, ix, d);
  out[0] = out[1] = -1;
  *tau2 = INFINITY;
  *d2min = INFINITY;
  for (int i = 0; i < n; ++i) {
    if (t[i] < *tau2) { *tau2 = t[i]; out[0] = i; out[1] = ix[i]; }
    if (d[i] < *d2min) *d2min = d[i];
  }
  free(t);
  free(d);
  free(ix);
}

void min_timescale_f64(const double *pos, const double *vel, int n, double *tau2, int *out, double *d2min) {
  double *t = (double *)malloc((size_t)n * sizeof(double)), *d = (double *)malloc((size_t)n * sizeof(double));
  int *ix = (int *)malloc((size_t)n * sizeof(int));
  timescale_f64(pos, vel, n, 0, n, t, ix, d);
  out[0] = out[1] = -1;
  *tau2 = INFINITY;
  *d2min = INFINITY;
  for (int i = 0; i < n; ++i) {
    if (t[i] < *tau2) { *tau2 = t[i]; out[0] = i; out[1] = ix[i]; }
    if (d[i] < *d2min) *d2min = d[i];
  }
  free(t);
  free(d);
  free(ix);
}
