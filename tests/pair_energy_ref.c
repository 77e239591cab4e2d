/* pair_energy_ref.c — an independent CPU statement of include/nbody.h ("pair binding energies and binaries"): per row i one ascending
 * scan over the bodies j != i,
 *   dx = xj - xi, dy = yj - yi, dz = zj - zi;        d2 = fma(dx, dx, fma(dy, dy, dz * dz))      (the context precision)
 *   ux = vxj - vxi, uy = vyj - vyi, uz = vzj - vzi;  v2 = fma(ux, ux, fma(uy, uy, uz * uz))
 *   s = d2 + eps;  inv = (float)(1.0 / sqrt((double)s))  (binary64: 1.0 / sqrt(s));  e = fma(0.5, v2, -2 * inv)
 * from (e = +inf, idx = -1), replacing on strict < (so the lowest j wins a tie and neither a NaN nor a +inf is ever chosen).  The system
 * form lists, in ascending i, the pairs i < j with idx[i] == j, idx[j] == i and e[i] < e_max, and computes their elements in binary64 in
 * the order the header gives.  Test infrastructure, compiled by the pair-energy tests with -ffp-contract=off (products are fused only
 * where fmaf / fma says so); rows are independent, so an OpenMP build changes nothing. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

static float eps32(void) {
  const unsigned bits = 0x3089705Fu;   /* the force's eps (include/nbody.h) */
  float e;
  memcpy(&e, &bits, sizeof(e));
  return e;
}

/* pos, vel: n words of 4 floats.  Rows first .. first + m - 1.  e, idx: m values each. */
void pair_energy_f32(const float *pos, const float *vel, int n, int first, int m, float *e, int *idx) {
  const float eps = eps32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const int i = first + p;
    const float x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    const float vx = vel[4 * (size_t)i], vy = vel[4 * (size_t)i + 1], vz = vel[4 * (size_t)i + 2];
    float best = INFINITY;
    int bi = -1;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const float dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const float ux = vel[4 * (size_t)j] - vx, uy = vel[4 * (size_t)j + 1] - vy, uz = vel[4 * (size_t)j + 2] - vz;
      const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      const float v2 = fmaf(ux, ux, fmaf(uy, uy, uz * uz));
      const float s = d2 + eps;
      const float inv = (float)(1.0 / sqrt((double)s));
      const float q = fmaf(0.5f, v2, -2.0f * inv);
      if (q < best) { best = q; bi = j; }
    }
    e[p] = best;
    idx[p] = bi;
  }
}

/* the same with words of 4 doubles */
void pair_energy_f64(const double *pos, const double *vel, int n, int first, int m, double *e, int *idx) {
  const double eps = (double)eps32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int p = 0; p < m; ++p) {
    const int i = first + p;
    const double x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    const double vx = vel[4 * (size_t)i], vy = vel[4 * (size_t)i + 1], vz = vel[4 * (size_t)i + 2];
    double best = INFINITY;
    int bi = -1;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const double dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const double ux = vel[4 * (size_t)j] - vx, uy = vel[4 * (size_t)j + 1] - vy, uz = vel[4 * (size_t)j + 2] - vz;
      const double d2 = fma(dx, dx, fma(dy, dy, dz * dz));
      const double v2 = fma(ux, ux, fma(uy, uy, uz * uz));
      const double s = d2 + eps;
      const double inv = 1.0 / sqrt(s);
      const double q = fma(0.5, v2, -2.0 * inv);
      if (q < best) { best = q; bi = j; }
    }
    e[p] = best;
    idx[p] = bi;
  }
}

/* one ordered pair's e alone (the symmetry test): row i against body j */
float pair_e_f32(const float *pos, const float *vel, int i, int j) {
  const float dx = pos[4 * j] - pos[4 * i], dy = pos[4 * j + 1] - pos[4 * i + 1], dz = pos[4 * j + 2] - pos[4 * i + 2];
  const float ux = vel[4 * j] - vel[4 * i], uy = vel[4 * j + 1] - vel[4 * i + 1], uz = vel[4 * j + 2] - vel[4 * i + 2];
  const float s = fmaf(dx, dx, fmaf(dy, dy, dz * dz)) + eps32();
  return fmaf(0.5f, fmaf(ux, ux, fmaf(uy, uy, uz * uz)), -2.0f * (float)(1.0 / sqrt((double)s)));
}
double pair_e_f64(const double *pos, const double *vel, int i, int j) {
  const double dx = pos[4 * j] - pos[4 * i], dy = pos[4 * j + 1] - pos[4 * i + 1], dz = pos[4 * j + 2] - pos[4 * i + 2];
  const double ux = vel[4 * j] - vel[4 * i], uy = vel[4 * j + 1] - vel[4 * i + 1], uz = vel[4 * j + 2] - vel[4 * i + 2];
  const double s = fma(dx, dx, fma(dy, dy, dz * dz)) + (double)eps32();
  return fma(0.5, fma(ux, ux, fma(uy, uy, uz * uz)), -2.0 * (1.0 / sqrt(s)));
}

/* {E, a, ecc, period} of a pair from its members' state in binary64 (r: 3 doubles each) */
void binary_elements(const double *ri, const double *rj, const double *vi, const double *vj, double *out) {
  const double dx = rj[0] - ri[0], dy = rj[1] - ri[1], dz = rj[2] - ri[2];
  const double ux = vj[0] - vi[0], uy = vj[1] - vi[1], uz = vj[2] - vi[2];
  const double s = ((dx * dx + dy * dy) + dz * dz) + (double)eps32();
  const double r = sqrt(s);
  const double v2 = (ux * ux + uy * uy) + uz * uz;
  const double E = 0.5 * v2 - 2.0 / r;
  const double a = -1.0 / E;
  const double cx = dy * uz - dz * uy, cy = dz * ux - dx * uz, cz = dx * uy - dy * ux;
  const double L2 = (cx * cx + cy * cy) + cz * cz;
  const double k = 1.0 + (0.5 * E) * L2;
  out[0] = E;
  out[1] = a;
  out[2] = sqrt(k > 0.0 ? k : 0.0);
  out[3] = 3.14159265358979323846 * sqrt(((2.0 * a) * a) * a);
}

/* the system form: returns the number of pairs found; the first min(found, max_pairs) into pi, pj, elements[4 k ..] */
int binaries_f32(const float *pos, const float *vel, int n, double e_max, int max_pairs, int *pi, int *pj, double *elements) {
  float *e = (float *)malloc((size_t)n * sizeof(float));
  int *ix = (int *)malloc((size_t)n * sizeof(int));
  int found = 0;
  pair_energy_f32(pos, vel, n, 0, n, e, ix);
  for (int i = 0; i < n; ++i) {
    const int j = ix[i];
    if (j <= i || ix[j] != i || !((double)e[i] < e_max)) continue;
    if (found < max_pairs) {
      double ri[3], rj[3], vi[3], vj[3];
      for (int c = 0; c < 3; ++c) {
        ri[c] = (double)pos[4 * (size_t)i + c]; rj[c] = (double)pos[4 * (size_t)j + c];
        vi[c] = (double)vel[4 * (size_t)i + c]; vj[c] = (double)vel[4 * (size_t)j + c];
      }
      pi[found] = i;
      pj[found] = j;
      binary_elements(ri, rj, vi, vj, elements + 4 * (size_t)found);
    }
    ++found;
  }
  free(e);
  free(ix);
  return found;
}

int binaries_f64(const double *pos, const double *vel, int n, double e_max, int max_pairs, int *pi, int *pj, double *elements) {
  double *e = (double *)malloc((size_t)n * sizeof(double));
  int *ix = (int *)malloc((size_t)n * sizeof(int));
  int found = 0;
  pair_energy_f64(pos, vel, n, 0, n, e, ix);
  for (int i = 0; i < n; ++i) {
    const int j = ix[i];
    if (j <= i || ix[j] != i || !(e[i] < e_max)) continue;
    if (found < max_pairs) {
      pi[found] = i;
      pj[found] = j;
      binary_elements(pos + 4 * (size_t)i, pos + 4 * (size_t)j, vel + 4 * (size_t)i, vel + 4 * (size_t)j, elements + 4 * (size_t)found);
    }
    ++found;
  }
  free(e);
  free(ix);
  return found;
}
