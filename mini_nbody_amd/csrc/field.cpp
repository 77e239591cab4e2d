// field.cpp — nbody_field(_d): acceleration and potential of the bodies on the device at m points the caller brings (field.hip).  Host
// C++ only.  Flow (query_pass.hpp): reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings them), then per
// local its contiguous range of the points: upload, the launch (and the combine launch when the sources are split) on the local's
// compute stream, stream sync, copy back.  nbody_init_rank contexts: every rank evaluates the points IT was given on its own device; the
// call is collective only through complete_positions().
// The pass reads pos[cur] and writes only the Local's q_* and fd_* buffers: positions, velocities, arrival counters, partial forces, the
// captured step graph and the force-kernel timer stay as they were.  Nothing outside this file refers to it.
#include "query_pass.hpp"
#include "field_args.hpp"

using namespace nbf;

namespace nbi {

namespace {

// points [r.first, r.first + r.cnt) of the call on local L (uploaded; outputs left in fd_accel / fd_phi for the copy back)
int launch_field(Local& L, const void* points, const int* skip, const Range& r, bool want_accel, bool want_phi) {
  HIPC(hipSetDevice(L.device));
  const size_t wb = word_bytes(), es = elem_bytes();
  NBC(upload_queries(L, points, skip, r.first, r.cnt));
  if (want_accel) NBC(L.fd_accel.ensure((size_t)r.cnt * wb));
  if (want_phi) NBC(L.fd_phi.ensure((size_t)r.cnt * es));
  const int n_blocks = source_blocks();
  const SplitPlan plan = block_split("NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB", r.cnt, n_blocks, 4, es);
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(field_scratch_bytes((size_t)plan.batch, (size_t)n_blocks, es)));
  return for_batches(r.cnt, plan, [&](int b0, int m) {
    FieldArgs a;
    memset(&a, 0, sizeof(a));
    a.src = L.pos[L.cur];
    a.points = L.q_points.as<char>() + (size_t)b0 * wb;
    a.skip = skip ? L.q_skip.as<int>() + b0 : nullptr;
    a.accel = want_accel ? L.fd_accel.as<char>() + (size_t)b0 * wb : nullptr;
    a.phi = want_phi ? L.fd_phi.as<char>() + (size_t)b0 * es : nullptr;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<void>() : nullptr;
    a.n_src = g.n;
    a.m = m;
    a.n_blocks = n_blocks;
    a.chunk_blocks = plan.chunk_blocks;
    HIPC((hipError_t)nbl::launch_field_kernel(g.fp64, g.opt.arith, L.compute, plan.chunks, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_field_combine_kernel(g.fp64, L.compute, a));
    return NBODY_OK;
  });
}

int field_impl(const void* points, int m, const int* skip, void* accel, void* phi) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!points || m < 1 || (!accel && !phi)) return NBODY_ERR_ARG;
  NBC(check_skip(skip, m));
  NBC(reconfigure());
  NBC(complete_positions());
  return run_on_locals([&](int l) { return points_of(m, l); },
                       [&](Local& L, const Range& r) { return launch_field(L, points, skip, r, accel != nullptr, phi != nullptr); },
                       [&](Local& L, const Range& r) {
                         NBC(copy_out(accel, r.out, L.fd_accel, r.cnt, word_bytes()));
                         return copy_out(phi, r.out, L.fd_phi, r.cnt, elem_bytes());
                       });
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_field(const float* points, int m, const int* skip, float* accel, float* phi) { NB_ENTER(0);
  return field_impl(points, m, skip, accel, phi);
}
int nbody_field_d(const double* points, int m, const int* skip, double* accel, double* phi) { NB_ENTER(1);
  return field_impl(points, m, skip, accel, phi);
}

}  // extern "C"
