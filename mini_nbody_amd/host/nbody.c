/* nbody.c — the host program, in C, over the C-ABI of include/nbody.h
 * (north_star: "host code stays in C ... calling hand-written HIP kernels
 * through a thin C-ABI shim").  The reference tree holds no host program
 * (SURVEY.md §0); this is the build's own: deterministic initial conditions,
 * the bodyForce()/integrate() loop or the device-resident step loop, timing
 * with the first iteration excluded as warm-up, and the metric of BASELINE.md
 * §2: billion pair-interactions/s = N^2 * timed_steps / seconds / 1e9.
 *
 * usage: nbody [N] [iters] [--gpus P] [--fp64] [--tile T] [--host-loop] [--seed S] [--strict] [--rtl] [--jsub K]
 *              [--sum seq|blocked] [--block K] [--one-launch | --two-launch] [--long-buffers 0|1] [--overlap 0|1|2] [--wsplit 1|4|16]
 *              [--energy] [--field M] [--tidal M] [--jerk M] [--closest-pair] [--pair-histogram B] [--adaptive ETA] [--binaries] [--hermite] [--hermite6] [--hermite-block LEVELS] [--hermite6-block LEVELS] [--masses]
 * --hermite: the device loop's iterations are fourth-order Hermite steps (nbody_step_hermite) instead of kick-drift steps: one warm-up
 * call of one step, the initial state uploaded again, then ONE timed call of all `iters` steps (a call opens with a jerk pass of its own,
 * so two calls would not be one run: include/nbody.h, "a call is stateless"); the time per step is that call's over iters.  Refused
 * together with --host-loop.
 * --hermite6: as --hermite, with sixth-order Hermite steps (nbody_step_hermite6: a call opens with the two passes of nbody_snap_rows);
 * the loop is named "device Hermite-6", and the --energy lines are printed, the drift being what the higher order is for.
 * --hermite-block LEVELS (1 <= LEVELS <= 24): as --hermite, but an iteration is one block of dt_max = 0.01 with individual block time
 * steps on LEVELS levels and eta = 0.02 (nbody_step_hermite_block); one more line, "hermite block: LEVELS levels, S sub-steps, R row
 * evaluations (F of sub-steps x N)", gives the timed call's counters.  LEVELS = 1 is --hermite bit for bit.
 * --hermite6-block LEVELS (1 <= LEVELS <= 24): as --hermite-block, over the sixth-order scheme (nbody_step_hermite6_block): the loop is
 * named "device Hermite-6 block", the counters' line begins "hermite6 block:", and the --energy lines are printed as with --hermite6.
 * LEVELS = 1 is --hermite6 bit for bit.  Not together with --hermite6 or --hermite-block.
 * --masses (with --hermite, --hermite6, --hermite-block or --hermite6-block only; anything else is a usage error): body i gets the mass 2^-(i mod 4) in the w of its
 * position word — exact in both precisions and fixed by i alone — NBODY_OPT_MASSES is switched on, and the --energy lines are printed:
 * the weighted E, T and U before the first iteration and after the last.
 * --energy: E = T + U, T and U of the state on the device (nbody_energy) before the first iteration and after the last, and the
 * relative drift, outside the timed region.
 * --field M: after the last iteration, acceleration and potential of the state on the device (nbody_field) at M points — the position
 * words of an M-body system of the same initial conditions with seed 4242 — as plain ascending fp64 sums, outside the timed region.
 * --tidal M: after the last iteration, the tidal tensor of the state on the device (nbody_tidal) at the M points of --field M: its trace
 * and its six values {xx, yy, zz, xy, xz, yz} as plain ascending fp64 sums over the points, outside the timed region.
 * --jerk M (1 <= M <= N): after the last iteration, acceleration and jerk of rows 0 .. M - 1 of the state on the device
 * (nbody_jerk_rows), each as three plain ascending fp64 sums over the rows, outside the timed region.
 * --closest-pair: after the last iteration, the two bodies of the state on the device that are closest and their plain squared distance
 * (nbody_closest_pair), outside the timed region.
 * --pair-histogram B (1 <= B <= 32): after the last iteration, one line "pair histogram: c0 c1 ... c(B-1)", the number of unordered
 * pairs of the state on the device per bin of squared distance (nbody_pair_histogram), outside the timed region.  The B + 1 edges are
 * edges2[0] = 0 and edges2[b] = 2^(2 (b - B) + 4) for b >= 1: exact powers of two up to 16 in either precision.
 * --adaptive ETA (ETA > 0): after the last iteration, one line "min timescale: tau2 ... pair i j d2min ... dt ...": the smallest pair
 * crossing time squared of the state on the device, the pair that gives it and the smallest squared distance (nbody_min_timescale), and
 * the step dt = ETA * sqrt(min(tau2, tff2)) that nbody_step_adaptive would take unclamped, in fp64, outside the timed region.
 * --binaries: after the last iteration, one line "binaries: K", the number of mutually most bound pairs with a negative pair energy in
 * the state on the device (nbody_binaries, e_max = 0), then up to five lines "binary: i j a ecc period", those with the smallest
 * semi-major axis a in ascending order of a (equal a: the lower i first), outside the timed region.
 */
#define _POSIX_C_SOURCE 199309L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "nbody.h"
#include "nbody_ic.h"

static double now_s(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s failed: %s\n", #call, nbody_error_string(rc_)); return 1; } } while (0)

/* one line of --energy: E, T and U of the state on the device after `step` iterations; *e0 is set on the first call */
static int print_energy(int step, double *e0, int first) {
  double w[NBODY_ENERGY_WORDS];
  int rc = nbody_energy(w);
  if (rc) { fprintf(stderr, "nbody_energy failed: %s\n", nbody_error_string(rc)); return 1; }
  const double t = w[NBODY_ENERGY_KINETIC], u = w[NBODY_ENERGY_POTENTIAL], e = t + u;
  if (first) {
    *e0 = e;
    printf("energy at step %d: E %.17g T %.17g U %.17g\n", step, e, t, u);
  } else {
    printf("energy at step %d: E %.17g T %.17g U %.17g relative drift %.3e\n", step, e, t, u, (e - *e0) / (*e0 != 0.0 ? fabs(*e0) : 1.0));
  }
  return 0;
}

/* the line of --field: phi and the three components of a summed over m points, ascending, in fp64 */
#define FIELD_SEED 4242u
static int print_field(int m, int fp64) {
  const size_t words = (size_t)m * 4;
  double phi_sum = 0.0, a_sum[3] = { 0.0, 0.0, 0.0 };
  int rc;
  if (!fp64) {
    float *buf = (float *)malloc((3 * words + (size_t)m) * sizeof(float));
    if (!buf) return 3;
    float *pts = buf, *acc = buf + 2 * words, *phi = buf + 3 * words;   /* buf + words: the velocities the fill also writes */
    nbody_ic_fill_f32(pts, buf + words, (size_t)m, 0, (size_t)m, FIELD_SEED);
    rc = nbody_field(pts, m, NULL, acc, phi);
    for (int p = 0; p < m && !rc; ++p) {
      phi_sum += (double)phi[p];
      for (int c = 0; c < 3; ++c) a_sum[c] += (double)acc[4 * p + c];
    }
    free(buf);
  } else {
    double *buf = (double *)malloc((3 * words + (size_t)m) * sizeof(double));
    if (!buf) return 3;
    double *pts = buf, *acc = buf + 2 * words, *phi = buf + 3 * words;
    nbody_ic_fill_f64(pts, buf + words, (size_t)m, 0, (size_t)m, FIELD_SEED);
    rc = nbody_field_d(pts, m, NULL, acc, phi);
    for (int p = 0; p < m && !rc; ++p) {
      phi_sum += phi[p];
      for (int c = 0; c < 3; ++c) a_sum[c] += acc[4 * p + c];
    }
    free(buf);
  }
  if (rc) { fprintf(stderr, "nbody_field failed: %s\n", nbody_error_string(rc)); return 1; }
  printf("field of %d points: phi_sum %.17g a_sum %.17g %.17g %.17g\n", m, phi_sum, a_sum[0], a_sum[1], a_sum[2]);
  return 0;
}

/* the line of --tidal: the trace and the six values of the tidal tensor summed over the m points of --field, ascending, in fp64 */
static int print_tidal(int m, int fp64) {
  const size_t words = (size_t)m * 4;
  double trace_sum = 0.0, t_sum[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
  int rc;
  if (!fp64) {
    float *buf = (float *)malloc((2 * words + 6 * (size_t)m) * sizeof(float));
    if (!buf) return 3;
    float *pts = buf, *t = buf + 2 * words;   /* buf + words: the velocities the fill also writes */
    nbody_ic_fill_f32(pts, buf + words, (size_t)m, 0, (size_t)m, FIELD_SEED);
    rc = nbody_tidal(pts, m, NULL, t);
    for (int p = 0; p < m && !rc; ++p) {
      trace_sum += ((double)t[6 * p] + (double)t[6 * p + 1]) + (double)t[6 * p + 2];
      for (int c = 0; c < 6; ++c) t_sum[c] += (double)t[6 * p + c];
    }
    free(buf);
  } else {
    double *buf = (double *)malloc((2 * words + 6 * (size_t)m) * sizeof(double));
    if (!buf) return 3;
    double *pts = buf, *t = buf + 2 * words;
    nbody_ic_fill_f64(pts, buf + words, (size_t)m, 0, (size_t)m, FIELD_SEED);
    rc = nbody_tidal_d(pts, m, NULL, t);
    for (int p = 0; p < m && !rc; ++p) {
      trace_sum += (t[6 * p] + t[6 * p + 1]) + t[6 * p + 2];
      for (int c = 0; c < 6; ++c) t_sum[c] += t[6 * p + c];
    }
    free(buf);
  }
  if (rc) { fprintf(stderr, "nbody_tidal failed: %s\n", nbody_error_string(rc)); return 1; }
  printf("tidal of %d points: trace_sum %.17g t_sum %.17g %.17g %.17g %.17g %.17g %.17g\n", m, trace_sum, t_sum[0], t_sum[1], t_sum[2], t_sum[3],
         t_sum[4], t_sum[5]);
  return 0;
}

/* the line of --jerk: the three components of the acceleration and of the jerk summed over rows 0 .. m - 1, ascending, in fp64 */
static int print_jerk(int m, int fp64) {
  const size_t words = (size_t)m * 4;
  double a_sum[3] = { 0.0, 0.0, 0.0 }, j_sum[3] = { 0.0, 0.0, 0.0 };
  int rc;
  if (!fp64) {
    float *buf = (float *)malloc(2 * words * sizeof(float));
    if (!buf) return 3;
    float *acc = buf, *jerk = buf + words;
    rc = nbody_jerk_rows(0, m, acc, jerk);
    for (int p = 0; p < m && !rc; ++p)
      for (int c = 0; c < 3; ++c) { a_sum[c] += (double)acc[4 * p + c]; j_sum[c] += (double)jerk[4 * p + c]; }
    free(buf);
  } else {
    double *buf = (double *)malloc(2 * words * sizeof(double));
    if (!buf) return 3;
    double *acc = buf, *jerk = buf + words;
    rc = nbody_jerk_rows_d(0, m, acc, jerk);
    for (int p = 0; p < m && !rc; ++p)
      for (int c = 0; c < 3; ++c) { a_sum[c] += acc[4 * p + c]; j_sum[c] += jerk[4 * p + c]; }
    free(buf);
  }
  if (rc) { fprintf(stderr, "nbody_jerk_rows failed: %s\n", nbody_error_string(rc)); return 1; }
  printf("jerk of %d rows: a_sum %.17g %.17g %.17g j_sum %.17g %.17g %.17g\n", m, a_sum[0], a_sum[1], a_sum[2], j_sum[0], j_sum[1], j_sum[2]);
  return 0;
}

/* the line of --closest-pair */
static int print_closest_pair(int fp64) {
  int i = -1, j = -1, rc;
  double d2 = 0.0;
  if (!fp64) {
    float d2f = 0.0f;
    rc = nbody_closest_pair(&i, &j, &d2f);
    d2 = (double)d2f;
  } else {
    rc = nbody_closest_pair_d(&i, &j, &d2);
  }
  if (rc) { fprintf(stderr, "nbody_closest_pair failed: %s\n", nbody_error_string(rc)); return 1; }
  printf("closest pair: %d %d d2 %.17g\n", i, j, d2);
  return 0;
}

/* the line of --adaptive */
static int print_min_timescale(double eta, int fp64) {
  int i = -1, j = -1, rc;
  double tau2 = 0.0, d2min = 0.0;
  if (!fp64) {
    float tf = 0.0f, df = 0.0f;
    rc = nbody_min_timescale(&tf, &i, &j, &df);
    tau2 = (double)tf; d2min = (double)df;
  } else {
    rc = nbody_min_timescale_d(&tau2, &i, &j, &d2min);
  }
  if (rc) { fprintf(stderr, "nbody_min_timescale failed: %s\n", nbody_error_string(rc)); return 1; }
  const unsigned eps_bits = 0x3089705Fu;   /* the force's eps (include/nbody.h) */
  float eps;
  memcpy(&eps, &eps_bits, sizeof(eps));
  const double s = d2min + (double)eps, tff2 = s * sqrt(s) / 2.0;
  printf("min timescale: tau2 %.17g pair %d %d d2min %.17g dt %.17g\n", tau2, i, j, d2min, eta * sqrt(tau2 < tff2 ? tau2 : tff2));
  return 0;
}

/* the lines of --binaries */
static int print_binaries(void) {
  int found = 0, rc = nbody_binaries(0.0, 0, &found, NULL, NULL, NULL);
  if (rc) { fprintf(stderr, "nbody_binaries failed: %s\n", nbody_error_string(rc)); return 1; }
  printf("binaries: %d\n", found);
  if (found == 0) return 0;
  int *ij = (int *)malloc(2 * (size_t)found * sizeof(int));
  double *el = (double *)malloc((size_t)found * NBODY_BINARY_WORDS * sizeof(double));
  char *shown = (char *)calloc((size_t)found, 1);
  if (!ij || !el || !shown) { free(ij); free(el); free(shown); return 3; }
  int k = 0;
  rc = nbody_binaries(0.0, found, &k, ij, ij + found, el);
  if (rc) fprintf(stderr, "nbody_binaries failed: %s\n", nbody_error_string(rc));
  if (k > found) k = found;
  for (int line = 0; !rc && line < 5 && line < k; ++line) {
    int best = -1;
    for (int q = 0; q < k; ++q)   /* ascending q is ascending i: strict < keeps the lower i; a NaN a is never shown */
      if (!shown[q] && el[NBODY_BINARY_WORDS * q + 1] == el[NBODY_BINARY_WORDS * q + 1] &&
          (best < 0 || el[NBODY_BINARY_WORDS * q + 1] < el[NBODY_BINARY_WORDS * best + 1])) best = q;
    if (best < 0) break;
    shown[best] = 1;
    const double *w = el + NBODY_BINARY_WORDS * best;
    printf("binary: %d %d %.17g %.17g %.17g\n", ij[best], ij[found + best], w[1], w[2], w[3]);
  }
  free(ij); free(el); free(shown);
  return rc ? 1 : 0;
}

/* the line of --pair-histogram */
static int print_pair_histogram(int bins, int fp64) {
  long long pairs[NBODY_HIST_MAX_BINS];
  int rc;
  if (!fp64) {
    float e[NBODY_HIST_MAX_BINS + 1];
    e[0] = 0.0f;
    for (int b = 1; b <= bins; ++b) e[b] = ldexpf(1.0f, 2 * (b - bins) + 4);
    rc = nbody_pair_histogram(e, bins, pairs);
  } else {
    double e[NBODY_HIST_MAX_BINS + 1];
    e[0] = 0.0;
    for (int b = 1; b <= bins; ++b) e[b] = ldexp(1.0, 2 * (b - bins) + 4);
    rc = nbody_pair_histogram_d(e, bins, pairs);
  }
  if (rc) { fprintf(stderr, "nbody_pair_histogram failed: %s\n", nbody_error_string(rc)); return 1; }
  printf("pair histogram:");
  for (int b = 0; b < bins; ++b) printf(" %lld", pairs[b]);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  int n = 30000, iters = 10, gpus = 1, fp64 = 0, tile = 0, host_loop = 0, strict = 0, rtl = 0, npos = 0, jsub = 0, sum = -1, block = 0, two_launch = -1, long_buffers = -1, overlap = -1, wsplit = 0, energy = 0, field = 0, tidal = 0, jerk = 0, closest = 0, pair_hist = 0, binaries = 0, hermite = 0, hermite6 = 0, block_levels = 0, block4 = 0, block6 = 0, masses = 0;
  double e0 = 0.0, adaptive = 0.0;
  unsigned long long seed = NBODY_IC_DEFAULT_SEED;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--gpus") && a + 1 < argc) gpus = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--tile") && a + 1 < argc) tile = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--jsub") && a + 1 < argc) jsub = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--seed") && a + 1 < argc) seed = strtoull(argv[++a], NULL, 10);
    else if (!strcmp(argv[a], "--fp64")) fp64 = 1;
    else if (!strcmp(argv[a], "--host-loop")) host_loop = 1;
    else if (!strcmp(argv[a], "--hermite")) hermite = 1;
    else if (!strcmp(argv[a], "--hermite6")) hermite = hermite6 = 1;
    else if (!strcmp(argv[a], "--hermite-block") && a + 1 < argc) { hermite = block4 = 1; block_levels = atoi(argv[++a]); if (block_levels < 1 || block_levels > 24) { fprintf(stderr, "--hermite-block needs 1 <= LEVELS <= 24\n"); return 2; } }
    else if (!strcmp(argv[a], "--hermite6-block") && a + 1 < argc) { hermite = block6 = 1; block_levels = atoi(argv[++a]); if (block_levels < 1 || block_levels > 24) { fprintf(stderr, "--hermite6-block needs 1 <= LEVELS <= 24\n"); return 2; } }
    else if (!strcmp(argv[a], "--masses")) masses = 1;
    else if (!strcmp(argv[a], "--strict")) strict = 1;
    else if (!strcmp(argv[a], "--rtl")) rtl = 1;
    else if (!strcmp(argv[a], "--energy")) energy = 1;
    else if (!strcmp(argv[a], "--field") && a + 1 < argc) field = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--tidal") && a + 1 < argc) tidal = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--jerk") && a + 1 < argc) jerk = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--closest-pair")) closest = 1;
    else if (!strcmp(argv[a], "--pair-histogram") && a + 1 < argc) { pair_hist = atoi(argv[++a]); if (pair_hist < 1 || pair_hist > NBODY_HIST_MAX_BINS) { fprintf(stderr, "--pair-histogram needs 1 <= B <= %d\n", NBODY_HIST_MAX_BINS); return 2; } }
    else if (!strcmp(argv[a], "--adaptive") && a + 1 < argc) { adaptive = atof(argv[++a]); if (!(adaptive > 0.0) || adaptive > 1e300) { fprintf(stderr, "--adaptive needs ETA > 0\n"); return 2; } }
    else if (!strcmp(argv[a], "--binaries")) binaries = 1;
    else if (!strcmp(argv[a], "--two-launch")) two_launch = 1;
    else if (!strcmp(argv[a], "--one-launch")) two_launch = 0;
    else if (!strcmp(argv[a], "--overlap") && a + 1 < argc) overlap = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--long-buffers") && a + 1 < argc) long_buffers = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--wsplit") && a + 1 < argc) wsplit = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--sum") && a + 1 < argc) { ++a; sum = !strcmp(argv[a], "seq") ? NBODY_SUM_SEQ : NBODY_SUM_BLOCKED; }
    else if (!strcmp(argv[a], "--block") && a + 1 < argc) block = atoi(argv[++a]);
    else if (argv[a][0] != '-' && npos == 0) { n = atoi(argv[a]); npos++; }
    else if (argv[a][0] != '-' && npos == 1) { iters = atoi(argv[a]); npos++; }
    else { fprintf(stderr, "usage: %s [N] [iters] [--gpus P] [--fp64] [--tile T] [--host-loop] [--seed S] [--strict] [--rtl] [--jsub K] [--sum seq|blocked] [--block K] [--one-launch|--two-launch] [--long-buffers 0|1] [--overlap 0|1|2] [--wsplit 1|4|16] [--energy] [--field M] [--tidal M] [--jerk M] [--closest-pair] [--pair-histogram B] [--adaptive ETA] [--binaries] [--hermite] [--hermite6] [--hermite-block LEVELS] [--hermite6-block LEVELS] [--masses]\n", argv[0]); return 2; }
  }
  if (field < 0) { fprintf(stderr, "--field needs M >= 1\n"); return 2; }
  if (tidal < 0) { fprintf(stderr, "--tidal needs M >= 1\n"); return 2; }
  if (jerk < 0 || jerk > n) { fprintf(stderr, "--jerk needs 1 <= M <= N\n"); return 2; }
  if (hermite && host_loop) { fprintf(stderr, "--hermite runs the device loop: not together with --host-loop\n"); return 2; }
  if (masses && !hermite) { fprintf(stderr, "--masses needs --hermite or --hermite-block: the kick-drift step is unit-mass\n"); return 2; }
  if (block6 && (hermite6 || block4)) { fprintf(stderr, "--hermite6-block: not together with --hermite6 or --hermite-block\n"); return 2; }
  if (hermite6 && block_levels) { fprintf(stderr, "--hermite6 has a shared dt: not together with --hermite-block\n"); return 2; }
  if (masses || hermite6 || block6) energy = 1;
  if (n <= 0 || iters < 2) { fprintf(stderr, "need N > 0 and iters >= 2 (iteration 1 is warm-up)\n"); return 2; }
  const float dt = 0.01f;
  const size_t words = (size_t)n * 4;
  CHECK(nbody_init(n, gpus, fp64, tile));
  /* (a strict binary32 arithmetic is granted by the library only after every device of the context has proved the strict 1/sqrt for
     every positive normal binary32 — nbody_strict_proof, 10 ms per device; otherwise the option call fails and CHECK reports why) */
  if (strict) CHECK(nbody_set_option(NBODY_OPT_ARITH, NBODY_ARITH_STRICT));   /* IEEE-exact: bit-identical to the CPU oracle */
  if (rtl) {
    /* the RTL-faithful result: the reference's own five roundings for d2 (S/dxy.vhd:113-122, S/dzsoft.vhd:201-202,
       S/dxyz_soft.vhd:149-150), 1/sqrt rounded once, and its own summation — 16 interleaved partial sums per axis over ONE stream of all
       N sources, latched rotated, joined by the adder tree (S/fxyz.vhd:129-184, S/final_adder.vhd:88-104, S/top_level.vhd:233-254) */
    CHECK(nbody_set_option(NBODY_OPT_ARITH, NBODY_ARITH_REFERENCE_STRICT));
    CHECK(nbody_set_option(NBODY_OPT_SUM_ORDER, NBODY_SUM_FPGA16));
    CHECK(nbody_set_option(NBODY_OPT_JSUB, 1));
  }
  if (masses) CHECK(nbody_set_option(NBODY_OPT_MASSES, 1));                    /* m_j = the w of body j's position word */
  if (jsub > 0) CHECK(nbody_set_option(NBODY_OPT_JSUB, jsub));                 /* source segments (summation order) */
  if (sum >= 0) CHECK(nbody_set_option(NBODY_OPT_SUM_ORDER, sum));             /* one sequential sum per segment, or blocks */
  if (block > 0) CHECK(nbody_set_option(NBODY_OPT_SUM_BLOCK, block));
  if (two_launch >= 0) CHECK(nbody_set_option(NBODY_OPT_FUSE_COMBINE, !two_launch));   /* in-launch combine or separate kernel (same bits) */
  if (long_buffers >= 0) CHECK(nbody_set_option(NBODY_OPT_ISA_LONG_BUFFERS, long_buffers));
  if (wsplit > 0) CHECK(nbody_set_option(NBODY_OPT_WSPLIT, wsplit));              /* waves of a workgroup share rows and split the segment (4) or not (1) */
  if (overlap >= 0) CHECK(nbody_set_option(NBODY_OPT_OVERLAP, overlap));        /* multi-GPU: 0 gather first, 1 own slice then the rest, 2 per arriving slice */

  double total = 0.0;
  long long substeps = 0, row_evals = 0;
  const float block_eta = 0.02f;
  if (!fp64) {
    float *buf = (float *)malloc(2 * words * sizeof(float));
    if (!buf) return 3;
    BodySystem p = { buf, buf + words };
    nbody_ic_fill_f32(p.pos, p.vel, (size_t)n, 0, (size_t)n, seed);
    if (masses) for (int i = 0; i < n; ++i) p.pos[4 * (size_t)i + 3] = ldexpf(1.0f, -(i % 4));
    if (energy) { CHECK(nbody_upload(&p)); if (print_energy(0, &e0, 1)) return 1; }
    if (host_loop) {
      for (int it = 1; it <= iters; ++it) {
        double t0 = now_s();
        CHECK(bodyForce(p.pos, p.vel, dt, n));   /* compute interbody forces, kick */
        CHECK(integrate(p.pos, p.vel, dt, n));   /* drift */
        double t = now_s() - t0;
        if (it > 1) total += t;                  /* first iteration is warm-up */
      }
    } else if (hermite) {
      CHECK(nbody_upload(&p));
      if (block6) CHECK(nbody_step_hermite6_block(block_eta, dt, block_levels, 1, NULL, NULL));
      else if (block_levels) CHECK(nbody_step_hermite_block(block_eta, dt, block_levels, 1, NULL, NULL));
      else if (hermite6) CHECK(nbody_step_hermite6(dt, 1));
      else CHECK(nbody_step_hermite(dt, 1));   /* warm-up; the call returns with the state written */
      CHECK(nbody_upload(&p));
      double t0 = now_s();
      if (block6) CHECK(nbody_step_hermite6_block(block_eta, dt, block_levels, iters, &substeps, &row_evals));
      else if (block_levels) CHECK(nbody_step_hermite_block(block_eta, dt, block_levels, iters, &substeps, &row_evals));
      else if (hermite6) CHECK(nbody_step_hermite6(dt, iters));
      else CHECK(nbody_step_hermite(dt, iters));
      total = now_s() - t0;
      CHECK(nbody_download(&p));
    } else {
      CHECK(nbody_upload(&p));
      CHECK(nbody_step(dt, 1));
      CHECK(nbody_sync());
      double t0 = now_s();
      CHECK(nbody_step(dt, iters - 1));
      CHECK(nbody_sync());
      total = now_s() - t0;
      CHECK(nbody_download(&p));
    }
    if ((energy || field || tidal || jerk || closest || pair_hist || binaries || adaptive > 0.0) && host_loop) CHECK(nbody_upload(&p));
    if (energy && print_energy(iters, &e0, 0)) return 1;
    if (field && print_field(field, 0)) return 1;
    if (tidal && print_tidal(tidal, 0)) return 1;
    if (jerk && print_jerk(jerk, 0)) return 1;
    if (closest && print_closest_pair(0)) return 1;
    if (pair_hist && print_pair_histogram(pair_hist, 0)) return 1;
    if (adaptive > 0.0 && print_min_timescale(adaptive, 0)) return 1;
    if (binaries && print_binaries()) return 1;
    double cx = 0, cy = 0, cz = 0;
    for (int i = 0; i < n; ++i) { cx += p.pos[4 * i]; cy += p.pos[4 * i + 1]; cz += p.pos[4 * i + 2]; }
    printf("checksum (sum of positions): %.9g %.9g %.9g\n", cx, cy, cz);
    free(buf);
  } else {
    double *buf = (double *)malloc(2 * words * sizeof(double));
    if (!buf) return 3;
    BodySystemD p = { buf, buf + words };
    nbody_ic_fill_f64(p.pos, p.vel, (size_t)n, 0, (size_t)n, seed);
    if (masses) for (int i = 0; i < n; ++i) p.pos[4 * (size_t)i + 3] = ldexp(1.0, -(i % 4));
    if (energy) { CHECK(nbody_upload_d(&p)); if (print_energy(0, &e0, 1)) return 1; }
    if (host_loop) {
      for (int it = 1; it <= iters; ++it) {
        double t0 = now_s();
        CHECK(bodyForce_d(p.pos, p.vel, dt, n));
        CHECK(integrate_d(p.pos, p.vel, dt, n));
        double t = now_s() - t0;
        if (it > 1) total += t;
      }
    } else if (hermite) {
      CHECK(nbody_upload_d(&p));
      if (block6) CHECK(nbody_step_hermite6_block_d(block_eta, dt, block_levels, 1, NULL, NULL));
      else if (block_levels) CHECK(nbody_step_hermite_block_d(block_eta, dt, block_levels, 1, NULL, NULL));
      else if (hermite6) CHECK(nbody_step_hermite6_d(dt, 1));
      else CHECK(nbody_step_hermite_d(dt, 1));
      CHECK(nbody_upload_d(&p));
      double t0 = now_s();
      if (block6) CHECK(nbody_step_hermite6_block_d(block_eta, dt, block_levels, iters, &substeps, &row_evals));
      else if (block_levels) CHECK(nbody_step_hermite_block_d(block_eta, dt, block_levels, iters, &substeps, &row_evals));
      else if (hermite6) CHECK(nbody_step_hermite6_d(dt, iters));
      else CHECK(nbody_step_hermite_d(dt, iters));
      total = now_s() - t0;
      CHECK(nbody_download_d(&p));
    } else {
      CHECK(nbody_upload_d(&p));
      CHECK(nbody_step_d(dt, 1));
      CHECK(nbody_sync());
      double t0 = now_s();
      CHECK(nbody_step_d(dt, iters - 1));
      CHECK(nbody_sync());
      total = now_s() - t0;
      CHECK(nbody_download_d(&p));
    }
    if ((energy || field || tidal || jerk || closest || pair_hist || binaries || adaptive > 0.0) && host_loop) CHECK(nbody_upload_d(&p));
    if (energy && print_energy(iters, &e0, 0)) return 1;
    if (field && print_field(field, 1)) return 1;
    if (tidal && print_tidal(tidal, 1)) return 1;
    if (jerk && print_jerk(jerk, 1)) return 1;
    if (closest && print_closest_pair(1)) return 1;
    if (pair_hist && print_pair_histogram(pair_hist, 1)) return 1;
    if (adaptive > 0.0 && print_min_timescale(adaptive, 1)) return 1;
    if (binaries && print_binaries()) return 1;
    double cx = 0, cy = 0, cz = 0;
    for (int i = 0; i < n; ++i) { cx += p.pos[4 * i]; cy += p.pos[4 * i + 1]; cz += p.pos[4 * i + 2]; }
    printf("checksum (sum of positions): %.17g %.17g %.17g\n", cx, cy, cz);
    free(buf);
  }
  if (block_levels)
    printf("%s block: %d levels, %lld sub-steps, %lld row evaluations (%.4f of sub-steps x N)\n", block6 ? "hermite6" : "hermite", block_levels, substeps, row_evals,
           (double)row_evals / ((double)substeps * (double)n));
  double avg = total / (double)(hermite ? iters : iters - 1);
  long long info_r = 0, info_s = 0, info_b = 0, info_l = 0, info_w = 0;
  nbody_get_info(NBODY_INFO_WSPLIT, &info_w);
  nbody_get_info(NBODY_INFO_IBLOCK, &info_r);
  nbody_get_info(NBODY_INFO_NSEG, &info_s);
  nbody_get_info(NBODY_INFO_SUM_BLOCK, &info_b);
  nbody_get_info(NBODY_INFO_LAUNCHES_PER_STEP, &info_l);
  printf("%d Bodies (%s, %d GPU%s, %s loop, %lld bodies/lane, %lld segments x %lld pieces, sum block %lld, %lld launch%s/step): average %0.3f Billion Interactions / second (%.3f ms / step)\n",
         n, fp64 ? "fp64" : "fp32", gpus, gpus > 1 ? "s" : "", host_loop ? "host" : block6 ? "device Hermite-6 block" : block_levels ? "device Hermite block" : hermite6 ? "device Hermite-6" : hermite ? "device Hermite" : "device", info_r, info_s, info_w, info_b, info_l,
         info_l > 1 ? "es" : "", 1e-9 * (double)n * (double)n / avg, 1e3 * avg);
  nbody_shutdown();
  return 0;
}
