// field.cpp — nbody_field(_d): acceleration and potential of the bodies on the device at m points the caller brings (field.hip).  Host
// C++ only.  Flow, as energy.cpp's: reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings them), then per
// local its contiguous range of the points: upload, the launch (and the combine launch when the sources are split) on the local's
// compute stream, stream sync, copy back.  nbody_init_rank contexts: every rank evaluates the points IT was given on its own device; the
// call is collective only through complete_positions().
// The pass reads pos[cur] and writes only the Local's fd_* buffers: positions, velocities, arrival counters, partial forces, the
// captured step graph and the force-kernel timer stay as they were.  Nothing outside this file refers to it.
#include "nbody_internal.hpp"
#include "field_args.hpp"

using namespace nbf;

namespace nbi {

namespace {

// Workgroups the launch should have before the sources stop being split, in units of the CU count (see choose_chunks): the starting
// value, not measured yet (tools/field_rate.py times the pass with and without the split).
constexpr int kFieldFill = 2;

long long env_ll(const char* name, long long dflt) {
  const char* e = getenv(name);
  return e && *e ? atoll(e) : dflt;
}

// C, the number of source chunks (grid.y) of a launch of `points` points over n_blocks blocks.  forced >= 1 (NBODY_FIELD_SPLIT):
// min(forced, n_blocks).  Auto: 1 when the points alone give kFieldFill workgroups per CU, else the smallest number of chunks that does.
int choose_chunks(long long forced, int points, int n_blocks) {
  if (forced >= 1) return (int)std::min<long long>(forced, n_blocks);
  const long long groups = ((long long)points + kFieldPoints - 1) / kFieldPoints;
  const long long want = (long long)kFieldFill * std::max(1, g.cu_count);
  if (groups >= want) return 1;
  return (int)std::min<long long>((want + groups - 1) / groups, n_blocks);
}

// points [p0, p0 + cnt) of the call on local L (uploaded; outputs left in fd_accel / fd_phi for copy_back)
int launch_field(Local& L, const void* points, const int* skip, int p0, int cnt, bool want_accel, bool want_phi) {
  HIPC(hipSetDevice(L.device));
  const size_t wb = word_bytes(), es = g.fp64 ? sizeof(double) : sizeof(float);
  NBC(L.fd_points.ensure((size_t)cnt * wb));
  HIPC(hipMemcpy(L.fd_points, (const char*)points + (size_t)p0 * wb, (size_t)cnt * wb, hipMemcpyHostToDevice));
  if (skip) {
    NBC(L.fd_skip.ensure((size_t)cnt * sizeof(int)));
    HIPC(hipMemcpy(L.fd_skip, skip + p0, (size_t)cnt * sizeof(int), hipMemcpyHostToDevice));
  }
  if (want_accel) NBC(L.fd_accel.ensure((size_t)cnt * wb));
  if (want_phi) NBC(L.fd_phi.ensure((size_t)cnt * es));

  const int n_blocks = (g.n + kFieldBlock - 1) / kFieldBlock;
  const long long forced = env_ll("NBODY_FIELD_SPLIT", 0);
  const long long bound = std::max<long long>(0, env_ll("NBODY_FIELD_SCRATCH_MB", 256)) << 20;
  // points whose per-block sums fit the scratch bound, in whole workgroups
  const long long fit = bound / (long long)field_scratch_bytes(1, (size_t)n_blocks, es) / kFieldPoints * kFieldPoints;
  int batch = cnt;
  if (choose_chunks(forced, cnt, n_blocks) > 1 && fit < cnt) batch = (int)fit;   // (fit < 256: batch = 0, no split)
  const int chunks = batch > 0 ? choose_chunks(forced, batch, n_blocks) : 1;
  if (chunks <= 1) batch = cnt;
  if (chunks > 1) NBC(L.fd_scratch.ensure(field_scratch_bytes((size_t)batch, (size_t)n_blocks, es)));

  for (int b0 = 0; b0 < cnt; b0 += batch) {
    FieldArgs a;
    memset(&a, 0, sizeof(a));
    a.src = L.pos[L.cur];
    a.points = L.fd_points.as<char>() + (size_t)b0 * wb;
    a.skip = skip ? L.fd_skip.as<int>() + b0 : nullptr;
    a.accel = want_accel ? L.fd_accel.as<char>() + (size_t)b0 * wb : nullptr;
    a.phi = want_phi ? L.fd_phi.as<char>() + (size_t)b0 * es : nullptr;
    a.scratch = chunks > 1 ? L.fd_scratch.as<void>() : nullptr;
    a.n_src = g.n;
    a.m = std::min(batch, cnt - b0);
    a.n_blocks = n_blocks;
    a.chunk_blocks = (n_blocks + chunks - 1) / chunks;
    const int grid_y = (n_blocks + a.chunk_blocks - 1) / a.chunk_blocks;   // no empty chunk
    HIPC((hipError_t)nbl::launch_field_kernel(g.fp64, g.opt.arith, L.compute, grid_y, a));
    if (chunks > 1) HIPC((hipError_t)nbl::launch_field_combine_kernel(g.fp64, L.compute, a));
  }
  return NBODY_OK;
}

int field_impl(const void* points, int m, const int* skip, void* accel, void* phi) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!points || m < 1 || (!accel && !phi)) return NBODY_ERR_ARG;
  if (skip)
    for (int p = 0; p < m; ++p)
      if (skip[p] < -1 || skip[p] >= g.n) return NBODY_ERR_ARG;
  NBC(reconfigure());
  NBC(complete_positions());
  const size_t wb = word_bytes(), es = g.fp64 ? sizeof(double) : sizeof(float);
  // the points in contiguous ranges over the locals (one local in an nbody_init_rank context: all of this rank's points)
  auto first_of = [&](int l) { return (int)((long long)m * l / g.nlocal); };
  for (int l = 0; l < g.nlocal; ++l) {
    const int p0 = first_of(l), cnt = first_of(l + 1) - p0;
    if (cnt > 0) NBC(launch_field(g.loc[l], points, skip, p0, cnt, accel != nullptr, phi != nullptr));
  }
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    const int p0 = first_of(l), cnt = first_of(l + 1) - p0;
    if (cnt <= 0) continue;
    HIPC(hipSetDevice(L.device));
    HIPC(hipStreamSynchronize(L.compute));   // then blocking copies into the caller's pageable memory, as the other entry points do
    if (accel) HIPC(hipMemcpy((char*)accel + (size_t)p0 * wb, L.fd_accel, (size_t)cnt * wb, hipMemcpyDeviceToHost));
    if (phi) HIPC(hipMemcpy((char*)phi + (size_t)p0 * es, L.fd_phi, (size_t)cnt * es, hipMemcpyDeviceToHost));
  }
  return NBODY_OK;
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_field(const float* points, int m, const int* skip, float* accel, float* phi) { NB_REFUSE_WHILE_SERVED();
  if (g.init && g.fp64) return NBODY_ERR_STATE;
  return field_impl(points, m, skip, accel, phi);
}
int nbody_field_d(const double* points, int m, const int* skip, double* accel, double* phi) { NB_REFUSE_WHILE_SERVED();
  if (g.init && !g.fp64) return NBODY_ERR_STATE;
  return field_impl(points, m, skip, accel, phi);
}

}  // extern "C"
