// tidal.cpp — nbody_tidal(_d): the tidal tensor of the bodies on the device at m points the caller brings (tidal.hip).  Host C++ only,
// in the shape of field.cpp.  Flow (query_pass.hpp): reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings
// them), then per local its contiguous range of the points: upload, the launch (and the combine launch when the sources are split) on
// the local's compute stream, stream sync, copy back.  nbody_init_rank contexts: every rank evaluates the points IT was given on its own
// device; the call is collective only through complete_positions().
// The pass reads pos[cur] and writes only the Local's q_* buffers and td_tensor: positions, velocities, arrival counters, partial forces,
// the captured step graph and the force-kernel timer stay as they were.  Nothing outside this file refers to it.
#include "query_pass.hpp"
#include "tidal_args.hpp"

using namespace nbt;

namespace nbi {

namespace {

// points [r.first, r.first + r.cnt) of the call on local L (uploaded; the six values per point left in td_tensor for the copy back)
int launch_tidal(Local& L, const void* points, const int* skip, const Range& r) {
  HIPC(hipSetDevice(L.device));
  const size_t wb = word_bytes(), es = elem_bytes();
  NBC(upload_queries(L, points, skip, r.first, r.cnt));
  NBC(L.td_tensor.ensure((size_t)r.cnt * kOut * es));
  const int n_blocks = source_blocks();
  const SplitPlan plan = block_split("NBODY_TIDAL_SPLIT", "NBODY_TIDAL_SCRATCH_MB", r.cnt, n_blocks, kSums, es);
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(tidal_scratch_bytes((size_t)plan.batch, (size_t)n_blocks, es)));
  return for_batches(r.cnt, plan, [&](int b0, int m) {
    TidalArgs a;
    memset(&a, 0, sizeof(a));
    a.src = L.pos[L.cur];
    a.points = L.q_points.as<char>() + (size_t)b0 * wb;
    a.skip = skip ? L.q_skip.as<int>() + b0 : nullptr;
    a.tensor = L.td_tensor.as<char>() + (size_t)b0 * kOut * es;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<void>() : nullptr;
    a.n_src = g.n;
    a.m = m;
    a.n_blocks = n_blocks;
    a.chunk_blocks = plan.chunk_blocks;
    HIPC((hipError_t)nbl::launch_tidal_kernel(g.fp64, g.opt.arith, L.compute, plan.chunks, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_tidal_combine_kernel(g.fp64, L.compute, a));
    return NBODY_OK;
  });
}

int tidal_impl(const void* points, int m, const int* skip, void* tensor) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!points || !tensor || m < 1) return NBODY_ERR_ARG;
  NBC(check_skip(skip, m));
  NBC(reconfigure());
  NBC(complete_positions());
  return run_on_locals([&](int l) { return points_of(m, l); },
                       [&](Local& L, const Range& r) { return launch_tidal(L, points, skip, r); },
                       [&](Local& L, const Range& r) { return copy_out(tensor, r.out, L.td_tensor, r.cnt, kOut * elem_bytes()); });
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_tidal(const float* points, int m, const int* skip, float* tensor) { NB_ENTER(0);
  return tidal_impl(points, m, skip, tensor);
}
int nbody_tidal_d(const double* points, int m, const int* skip, double* tensor) { NB_ENTER(1);
  return tidal_impl(points, m, skip, tensor);
}

}  // extern "C"
