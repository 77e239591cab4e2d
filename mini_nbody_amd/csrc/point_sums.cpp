// point_sums.cpp — nbody_field(_d), nbody_tidal(_d), nbody_jerk(_d), nbody_jerk_rows(_d), nbody_snap(_d) and nbody_snap_rows(_d): the
// field (acceleration and potential), the tidal tensor, the jerk and the snap of the bodies on the device at m points the caller brings,
// and the jerk and the snap at rows of the state itself (point_sums.hip).  Host C++ only; one flow, the pass (point_sums_args.hpp) and the queries say what differs.
// Flow (query_pass.hpp): reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings them), a pass with
// velocities then gather_velocities() (all N of them where every local's kernel can read them), then per local its contiguous range of
// the points — or its rows of the window, which are read where they lie: nothing is uploaded —: upload, the launch (and the combine
// launch when the sources are split) on the local's compute stream, stream sync, copy back.  nbody_init_rank contexts: every rank
// evaluates the points IT was given (its own rows) on its own device; the call is collective only through complete_positions() and
// gather_velocities().
// A call reads pos[cur] (and vel) and writes only the Local's q_* buffers (and ts_vel, full_scratch): positions, velocities, arrival
// counters, partial forces, the captured step graph and the force-kernel timer stay as they were.  Internal entries (query_pass.hpp)
// serve the Hermite integrators: jerk_own_rows_on_device the step of hermite.cpp, jerk_points_on_device the block step of
// hermite_block.cpp, snap_own_rows_on_device the step of hermite6.cpp, snap_points_on_device the block step of hermite6_block.cpp.
// The snap pass reads the sources' accelerations as a third stream.  A snap call makes them itself: the jerk rows pass over every
// local's own rows into sn_acc, then gather_accelerations() (all N of them to every device: sn_acc itself or sn_acc_all), then the snap
// pass; the sixth-order integrator (hermite6.cpp) brings predicted ones to snap_own_rows_on_device.
#include "query_pass.hpp"
#include "point_sums_args.hpp"

using namespace nbp;

namespace nbi {

namespace {

// The queries of a call.  Points: the caller's arrays in host memory (velocities: a pass with velocities only).  Rows (points ==
// null): the window's bodies themselves, each leaving itself out.  on_device: the three are the local's own q_points, q_vel and q_skip
// (accelerations: q_acc too), which a kernel has filled: nothing is uploaded.
struct Queries { const void* points; const void* velocities; const int* skip; bool on_device = false; const void* accelerations = nullptr; };
constexpr int kOuts = 3;   // out[0], out[1] and out2 of PointSumsArgs

// queries [r.first, r.first + r.cnt) of the call on local L — points of the call (uploaded) or rows of L's slice — with the outputs
// asked for left in q_out (the third in q_out2) for the copy back, or (dev) in the device buffers the caller names, which it has sized.
// acc_all: a pass with accelerations: all N of the sources' in L's device memory
DevMem& out_buffer(Local& L, int i) { return i < 2 ? L.q_out[i] : L.q_out2; }
size_t out_bytes(const PointPass& pass, int i) { return (size_t)(i < 2 ? pass.out_values[i] : pass.out2_values) * elem_bytes(); }   // per point

int launch_point_sums(Local& L, const PointPass& pass, const Queries& q, const Range& r, void* const (&out)[kOuts], bool dev = false,
                      const void* acc_all = nullptr) {
  HIPC(hipSetDevice(L.device));
  const size_t wb = word_bytes(), es = elem_bytes();
  const size_t ob[kOuts] = {out_bytes(pass, 0), out_bytes(pass, 1), out_bytes(pass, 2)};   // bytes per point of each output
  if (q.points && !q.on_device) NBC(upload_queries(L, q.points, q.skip, r.first, r.cnt, q.velocities, q.accelerations));
  char* base[kOuts];
  for (int i = 0; i < kOuts; ++i) {
    if (out[i] && !dev) NBC(out_buffer(L, i).ensure((size_t)r.cnt * ob[i]));
    base[i] = dev ? (char*)out[i] : out_buffer(L, i).as<char>();
  }
  const int n_blocks = source_blocks();
  const SplitPlan plan = block_split(pass.split_env, pass.scratch_mb_env, r.cnt, n_blocks, pass.sums, es);
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(point_sums_scratch_bytes((size_t)plan.batch, (size_t)n_blocks, (size_t)pass.sums, es)));
  return for_batches(r.cnt, plan, [&](int b0, int m) {
    PointSumsArgs a;
    memset(&a, 0, sizeof(a));
    a.src = L.pos[L.cur];
    if (pass.velocities) a.vsrc = velocities_of(L);
    if (q.points) {
      a.points = L.q_points.as<char>() + (size_t)b0 * wb;
      a.skip = q.skip ? L.q_skip.as<int>() + b0 : nullptr;
      if (q.velocities) a.pvel = L.q_vel.as<char>() + (size_t)b0 * wb;
      if (q.accelerations) a.pacc = L.q_acc.as<char>() + (size_t)b0 * wb;
    } else {
      a.first = L.first + r.first + b0;
    }
    for (int i = 0; i < 2; ++i) a.out[i] = out[i] ? base[i] + (size_t)b0 * ob[i] : nullptr;
    a.out2 = out[2] ? base[2] + (size_t)b0 * ob[2] : nullptr;
    if (pass.accelerations) a.asrc = acc_all;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<void>() : nullptr;
    a.n_src = g.n;
    a.m = m;
    a.n_blocks = n_blocks;
    a.chunk_blocks = plan.chunk_blocks;
    a.masses = g.opt.masses;
    HIPC((hipError_t)nbl::launch_point_sums_kernel(pass, g.fp64, g.opt.arith, L.compute, plan.chunks, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_point_sums_combine_kernel(pass, g.fp64, L.compute, a));
    return NBODY_OK;
  });
}

// the checked call: what every form does once its arguments hold.  range_of(l): local l's part of the queries
}  // namespace

// The sources' accelerations of a snap call (and of a sixth-order Hermite call's opening): the jerk rows pass over ALL N rows, every
// local its own into sn_acc, and the N words to every device (accelerations_of(L, &Local::sn_acc)).  The caller has made pos[cur]
// complete and gathered the velocities.  An nbody_init_rank job gathers the accelerations through full_scratch, where the velocities
// lay: those are brought again.
int snap_open_accelerations() {
  for (int l = 0; l < g.nlocal; ++l) {
    Local& L = g.loc[l];
    if (L.n_local <= 0) continue;
    HIPC(hipSetDevice(L.device));
    NBC(L.sn_acc.ensure((size_t)L.n_local * word_bytes()));
    NBC(jerk_own_rows_on_device(L, L.sn_acc, nullptr));
  }
  NBC(gather_accelerations(&Local::sn_acc));
  if (g.multiprocess && g.nranks > 1) NBC(gather_velocities());
  return NBODY_OK;
}

namespace {

template <typename RangeOf>
int run_point_sums(const PointPass& pass, const Queries& q, RangeOf&& range_of, void* const (&out)[kOuts]) {
  NBC(reconfigure());
  NBC(complete_positions());
  if (pass.velocities) NBC(gather_velocities());
  if (pass.accelerations) NBC(snap_open_accelerations());
  return run_on_locals(range_of,
                       [&](Local& L, const Range& r) {
                         return launch_point_sums(L, pass, q, r, out, false, pass.accelerations ? accelerations_of(L, &Local::sn_acc) : nullptr);
                       },
                       [&](Local& L, const Range& r) {
                         for (int i = 0; i < kOuts; ++i) NBC(copy_out(out[i], r.out, out_buffer(L, i), r.cnt, out_bytes(pass, i)));
                         return NBODY_OK;
                       });
}

// out: the caller's arrays, null where the pass has no such output or the caller does not ask for it; at least one
int point_sums_impl(const PointPass& pass, const void* points, const void* velocities, int m, const int* skip, void* out0, void* out1,
                    const void* accelerations = nullptr, void* out2 = nullptr) {
  void* const out[kOuts] = {out0, out1, out2};
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!points || (pass.velocities && !velocities) || (pass.accelerations && !accelerations) || m < 1 || (!out[0] && !out[1] && !out[2]))
    return NBODY_ERR_ARG;
  NBC(check_skip(skip, m));
  return run_point_sums(pass, {points, velocities, skip, false, accelerations}, [&](int l) { return points_of(m, l); }, out);
}

// the rows form of a pass with velocities: rows as nbody_timescale_rows takes them
int point_sums_rows_impl(const PointPass& pass, int first_row, int n_rows, void* out0, void* out1, void* out2 = nullptr) {
  void* const out[kOuts] = {out0, out1, out2};
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!out[0] && !out[1] && !out[2]) return NBODY_ERR_ARG;
  RowWindow w;   // rows as in nbody_forces_rows
  NBC(w.open(first_row, n_rows));
  return run_point_sums(pass, {nullptr, nullptr, nullptr}, [&](int l) { return rows_of(w, l); }, out);
}

}  // namespace

// The jerk rows pass over L's own rows into accel and jerk, n_local words each in L's device memory: the split and the batches of
// launch_point_sums, no copy back (hermite.cpp).  The caller has made pos[cur] complete and gathered the velocities; the launches are
// left on L's compute stream.
int jerk_own_rows_on_device(Local& L, void* accel, void* jerk) {
  if (L.n_local <= 0) return NBODY_OK;
  void* const out[kOuts] = {accel, jerk, nullptr};
  return launch_point_sums(L, kJerkPass, {nullptr, nullptr, nullptr}, {0, L.n_local, 0}, out, true);
}

// The snap rows pass over L's own rows likewise, into accel, jerk and snap (any may be null, not all).  acc_all: the accelerations of
// all N sources in L's device memory, the third source stream: the caller has gathered them too (hermite6.cpp: the predicted ones).
int snap_own_rows_on_device(Local& L, const void* acc_all, void* accel, void* jerk, void* snap) {
  if (L.n_local <= 0) return NBODY_OK;
  void* const out[kOuts] = {accel, jerk, snap};
  return launch_point_sums(L, kSnapPass, {nullptr, nullptr, nullptr}, {0, L.n_local, 0}, out, true, acc_all);
}

// The jerk points pass over m queries a kernel has left in L's q_points, q_vel and q_skip (the block step of hermite_block.cpp: the
// active rows' predicted words and global indices) into accel and jerk, m words each in L's device memory: the same split and batches,
// nothing uploaded, no copy back.  The caller has made pos[cur] complete and gathered the velocities; the launches are left on L's
// compute stream.
int jerk_points_on_device(Local& L, int m, void* accel, void* jerk) {
  if (m <= 0) return NBODY_OK;
  void* const out[kOuts] = {accel, jerk, nullptr};
  return launch_point_sums(L, kJerkPass, {L.q_points.as<void>(), L.q_vel.as<void>(), L.q_skip.as<int>(), true}, {0, m, 0}, out, true);
}

// The snap points pass likewise over m queries a kernel has left in L's q_points, q_vel, q_acc and q_skip (the sixth-order block step
// of hermite6_block.cpp: the active rows' predicted words and global indices) into accel, jerk and snap, m words each in L's device
// memory (any may be null, not all).  acc_all: the accelerations of all N sources in L's device memory, which the caller has gathered
// with the positions and the velocities.
int snap_points_on_device(Local& L, int m, const void* acc_all, void* accel, void* jerk, void* snap) {
  if (m <= 0) return NBODY_OK;
  void* const out[kOuts] = {accel, jerk, snap};
  return launch_point_sums(L, kSnapPass, {L.q_points.as<void>(), L.q_vel.as<void>(), L.q_skip.as<int>(), true, L.q_acc.as<void>()}, {0, m, 0},
                           out, true, acc_all);
}

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_field(const float* points, int m, const int* skip, float* accel, float* phi) { NB_ENTER(0);
  return point_sums_impl(kFieldPass, points, nullptr, m, skip, accel, phi);
}
int nbody_field_d(const double* points, int m, const int* skip, double* accel, double* phi) { NB_ENTER(1);
  return point_sums_impl(kFieldPass, points, nullptr, m, skip, accel, phi);
}
int nbody_tidal(const float* points, int m, const int* skip, float* tensor) { NB_ENTER(0);
  return point_sums_impl(kTidalPass, points, nullptr, m, skip, tensor, nullptr);
}
int nbody_tidal_d(const double* points, int m, const int* skip, double* tensor) { NB_ENTER(1);
  return point_sums_impl(kTidalPass, points, nullptr, m, skip, tensor, nullptr);
}
int nbody_jerk(const float* points, const float* velocities, int m, const int* skip, float* accel, float* jerk) { NB_ENTER(0);
  return point_sums_impl(kJerkPass, points, velocities, m, skip, accel, jerk);
}
int nbody_jerk_d(const double* points, const double* velocities, int m, const int* skip, double* accel, double* jerk) { NB_ENTER(1);
  return point_sums_impl(kJerkPass, points, velocities, m, skip, accel, jerk);
}
int nbody_jerk_rows(int first_row, int n_rows, float* accel, float* jerk) { NB_ENTER(0);
  return point_sums_rows_impl(kJerkPass, first_row, n_rows, accel, jerk);
}
int nbody_jerk_rows_d(int first_row, int n_rows, double* accel, double* jerk) { NB_ENTER(1);
  return point_sums_rows_impl(kJerkPass, first_row, n_rows, accel, jerk);
}
int nbody_snap(const float* points, const float* velocities, const float* accelerations, int m, const int* skip, float* accel, float* jerk,
               float* snap) { NB_ENTER(0);
  return point_sums_impl(kSnapPass, points, velocities, m, skip, accel, jerk, accelerations, snap);
}
int nbody_snap_d(const double* points, const double* velocities, const double* accelerations, int m, const int* skip, double* accel,
                 double* jerk, double* snap) { NB_ENTER(1);
  return point_sums_impl(kSnapPass, points, velocities, m, skip, accel, jerk, accelerations, snap);
}
int nbody_snap_rows(int first_row, int n_rows, float* accel, float* jerk, float* snap) { NB_ENTER(0);
  return point_sums_rows_impl(kSnapPass, first_row, n_rows, accel, jerk, snap);
}
int nbody_snap_rows_d(int first_row, int n_rows, double* accel, double* jerk, double* snap) { NB_ENTER(1);
  return point_sums_rows_impl(kSnapPass, first_row, n_rows, accel, jerk, snap);
}

}  // extern "C"
