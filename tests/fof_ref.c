/* fof_ref.c — an independent CPU statement of include/nbody.h ("friends-of-friends groups"): every pair i < j once,
 *   dx = xj - xi, dy = yj - yi, dz = zj - zi;  d2 = fma(dx, dx, fma(dy, dy, dz * dz))      (no softening; the context precision)
 * and where d2 <= b2 (a NaN d2 never is) the two bodies' sets united in a union-find whose root is always the lowest index; group[i]
 * is then the root of i's set, the lowest index of its connected component, whatever the order of the unions.  No rounds, no labels
 * handed about: O(N^2) pairs and nothing of the library's algorithm.  Test infrastructure, compiled by the fof tests with
 * -ffp-contract=off (products are fused only where fmaf / fma says so); the pairs are independent and the unions are taken one at a
 * time, so an OpenMP build changes nothing. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

static int find_root(int *parent, int i) {
  int r = i;
  while (parent[r] != r) r = parent[r];
  while (parent[i] != r) { const int up = parent[i]; parent[i] = r; i = up; }
  return r;
}

static void unite(int *parent, int a, int b) {
  a = find_root(parent, a);
  b = find_root(parent, b);
  if (a < b) parent[b] = a;
  else if (b < a) parent[a] = b;
}

/* pos: n words of 4 floats.  group: n ints.  Returns the number of groups. */
int fof_f32(const float *pos, int n, float b2, int *group) {
  for (int i = 0; i < n; ++i) group[i] = i;
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; ++i) {
    const float x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    for (int j = i + 1; j < n; ++j) {
      const float dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const float v = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      if (v <= b2) {
#pragma omp critical(fof_union)
        unite(group, i, j);
      }
    }
  }
  int roots = 0;
  for (int i = 0; i < n; ++i) {
    group[i] = find_root(group, i);
    roots += group[i] == i;
  }
  return roots;
}

/* the same with words of 4 doubles */
int fof_f64(const double *pos, int n, double b2, int *group) {
  for (int i = 0; i < n; ++i) group[i] = i;
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; ++i) {
    const double x = pos[4 * (size_t)i], y = pos[4 * (size_t)i + 1], z = pos[4 * (size_t)i + 2];
    for (int j = i + 1; j < n; ++j) {
      const double dx = pos[4 * (size_t)j] - x, dy = pos[4 * (size_t)j + 1] - y, dz = pos[4 * (size_t)j + 2] - z;
      const double v = fma(dx, dx, fma(dy, dy, dz * dz));
      if (v <= b2) {
#pragma omp critical(fof_union)
        unite(group, i, j);
      }
    }
  }
  int roots = 0;
  for (int i = 0; i < n; ++i) {
    group[i] = find_root(group, i);
    roots += group[i] == i;
  }
  return roots;
}
