/* potential_ref.c — an independent CPU statement of the potential of include/nbody.h ("energy and potential"), in its documented order:
 *   phi_i = 0 - S_i,  S_i = sum over blocks of 1024 sources ascending (fp64) of the block's sum from zero, ascending j, j != i, of
 *   (|r_j - r_i|^2 + eps)^(-1/2) in the context precision;  eps = the binary32 with bits 0x3089705F.
 * binary32: d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps))) or (ref) (dx*dx + dy*dy) + fmaf(dz, dz, eps), 1/sqrt as the IEEE value
 * (float)(1.0 / sqrt((double)d2)).  binary64: the fma-contracted d2, 1.0 / sqrt(d2).  Test infrastructure, compiled by
 * tests/test_gpu_energy.py with -ffp-contract=off (products are fused only where fmaf / fma says so); rows are independent, so an
 * OpenMP build changes no bit.
 * energy_totals_f32 / _f64 restate the header's order of the totals {T, U, Px, Py, Pz, Lx, Ly, Lz}: per slice (first, count) of rows — a
 * rank's — groups of 256 rows from the slice's first row, each summed from zero in ascending rows in binary64 from the binary64 values
 * (U from 0 - S_i, T from fma(vx, vx, fma(vy, vy, vz * vz)), L from y * vz - z * vy and its cyclic permutations with two rounded
 * products), the groups' sums added from zero in ascending order, T and U halved; then the slices' eight values added from zero in
 * slice order. */
#include <math.h>
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

/* pos: n words of 4 floats; phi[k] = phi of row r0 + k, k < nr; ref: the reference's d2 roundings */
void potential_f32(const float *pos, int n, int r0, int nr, int ref, float *phi) {
  const float eps = eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int k = 0; k < nr; ++k) {
    const int i = r0 + k;
    const float xi = pos[4 * i], yi = pos[4 * i + 1], zi = pos[4 * i + 2];
    double s2 = 0.0;
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      float s1 = 0.0f;
      for (int j = b0; j < b1; ++j) {
        if (j == i) continue;
        const float dx = pos[4 * j] - xi, dy = pos[4 * j + 1] - yi, dz = pos[4 * j + 2] - zi;
        float d2;
        if (ref) {
          const float sxy = dx * dx + dy * dy;
          d2 = sxy + fmaf(dz, dz, eps);
        } else {
          d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps)));
        }
        s1 += (float)(1.0 / sqrt((double)d2));
      }
      s2 += (double)s1;
    }
    phi[k] = (float)(0.0 - s2);
  }
}

/* pos: n words of 4 doubles */
void potential_f64(const double *pos, int n, int r0, int nr, double *phi) {
  const double eps = (double)eps_f32();
#pragma omp parallel for schedule(dynamic, 16)
  for (int k = 0; k < nr; ++k) {
    const int i = r0 + k;
    const double xi = pos[4 * i], yi = pos[4 * i + 1], zi = pos[4 * i + 2];
    double s2 = 0.0;
    for (int b0 = 0; b0 < n; b0 += BLOCK) {
      const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
      double s1 = 0.0;
      for (int j = b0; j < b1; ++j) {
        if (j == i) continue;
        const double dx = pos[4 * j] - xi, dy = pos[4 * j + 1] - yi, dz = pos[4 * j + 2] - zi;
        s1 += 1.0 / sqrt(fma(dx, dx, fma(dy, dy, fma(dz, dz, eps))));
      }
      s2 += s1;
    }
    phi[k] = 0.0 - s2;
  }
}

#define GROUP 256
#define WORDS 8

/* S_i before phi_i = 0 - S_i is rounded to the context precision: what the totals take U from */
static double s_row_f32(const float *pos, int n, int i, int ref) {
  const float eps = eps_f32();
  const float xi = pos[4 * i], yi = pos[4 * i + 1], zi = pos[4 * i + 2];
  double s2 = 0.0;
  for (int b0 = 0; b0 < n; b0 += BLOCK) {
    const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
    float s1 = 0.0f;
    for (int j = b0; j < b1; ++j) {
      if (j == i) continue;
      const float dx = pos[4 * j] - xi, dy = pos[4 * j + 1] - yi, dz = pos[4 * j + 2] - zi;
      float d2;
      if (ref) {
        const float sxy = dx * dx + dy * dy;
        d2 = sxy + fmaf(dz, dz, eps);
      } else {
        d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps)));
      }
      s1 += (float)(1.0 / sqrt((double)d2));
    }
    s2 += (double)s1;
  }
  return s2;
}

static double s_row_f64(const double *pos, int n, int i) {
  const double eps = (double)eps_f32();
  const double xi = pos[4 * i], yi = pos[4 * i + 1], zi = pos[4 * i + 2];
  double s2 = 0.0;
  for (int b0 = 0; b0 < n; b0 += BLOCK) {
    const int b1 = b0 + BLOCK < n ? b0 + BLOCK : n;
    double s1 = 0.0;
    for (int j = b0; j < b1; ++j) {
      if (j == i) continue;
      const double dx = pos[4 * j] - xi, dy = pos[4 * j + 1] - yi, dz = pos[4 * j + 2] - zi;
      s1 += 1.0 / sqrt(fma(dx, dx, fma(dy, dy, fma(dz, dz, eps))));
    }
    s2 += s1;
  }
  return s2;
}

/* the eight binary64 values of one row from its S_i and its binary64 position and velocity */
static void row_words(double s, double x, double y, double z, double vx, double vy, double vz, double *w) {
  w[0] = fma(vx, vx, fma(vy, vy, vz * vz));
  w[1] = 0.0 - s;
  w[2] = vx; w[3] = vy; w[4] = vz;
  w[5] = y * vz - z * vy;
  w[6] = z * vx - x * vz;
  w[7] = x * vy - y * vx;
}

/* w: n rows of 8 values; slices: nslices pairs {first, count}; out: 8 values */
static void totals_of(const double *w, const int *slices, int nslices, double *out) {
  for (int q = 0; q < WORDS; ++q) out[q] = 0.0;
  for (int r = 0; r < nslices; ++r) {
    const int first = slices[2 * r], end = first + slices[2 * r + 1];
    double tot[WORDS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g0 = first; g0 < end; g0 += GROUP) {
      const int g1 = g0 + GROUP < end ? g0 + GROUP : end;
      double acc[WORDS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int i = g0; i < g1; ++i)
        for (int q = 0; q < WORDS; ++q) acc[q] += w[(size_t)WORDS * i + q];
      for (int q = 0; q < WORDS; ++q) tot[q] += acc[q];
    }
    tot[0] = 0.5 * tot[0];
    tot[1] = 0.5 * tot[1];
    for (int q = 0; q < WORDS; ++q) out[q] += tot[q];
  }
}

/* pos, vel: n words of 4 floats; returns 0, or 1 without memory */
int energy_totals_f32(const float *pos, const float *vel, int n, const int *slices, int nslices, int ref, double *out) {
  double *w = (double *)malloc((size_t)n * WORDS * sizeof(double));
  if (!w) return 1;
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; ++i)
    row_words(s_row_f32(pos, n, i, ref), pos[4 * i], pos[4 * i + 1], pos[4 * i + 2], vel[4 * i], vel[4 * i + 1], vel[4 * i + 2],
              w + (size_t)WORDS * i);
  totals_of(w, slices, nslices, out);
  free(w);
  return 0;
}

/* pos, vel: n words of 4 doubles */
int energy_totals_f64(const double *pos, const double *vel, int n, const int *slices, int nslices, double *out) {
  double *w = (double *)malloc((size_t)n * WORDS * sizeof(double));
  if (!w) return 1;
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; ++i)
    row_words(s_row_f64(pos, n, i), pos[4 * i], pos[4 * i + 1], pos[4 * i + 2], vel[4 * i], vel[4 * i + 1], vel[4 * i + 2],
              w + (size_t)WORDS * i);
  totals_of(w, slices, nslices, out);
  free(w);
  return 0;
}
