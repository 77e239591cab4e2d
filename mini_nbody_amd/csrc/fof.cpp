// fof.cpp — nbody_fof(_d): friends-of-friends groups, the connected components of "d2_ij <= b2" (fof.hip).  Host C++ only.  The
// all-pairs work runs on the device, the O(N) bookkeeping here: a union-find over the N bodies whose root is always the lowest index,
// L[i] = find(i).  A ROUND uploads L to every local that has rows, runs the link pass — per active row the lowest FOREIGN label among
// its friends, kFoNone if there is none — copies the m_i back and unites i with m_i.  A round in which no row reported ends the call.
// A foreign label, not just a lower one: every group that is not yet a whole component has a row that reports, so every incomplete
// group is merged with another in every round, their number at least halves, and floor(log2 N) merging rounds and the final silent one
// are the most a call can take (round_cap; beyond it NBODY_ERR_STATE — nothing on the device ever spins or polls).  The link relation is
// symmetric bit for bit, so the groups a reporting group merged with reported too: a group none of whose rows reported is a finished
// component, and later rounds launch over the compacted list of the other groups' rows only (NBODY_FOF_ALL_ROWS=1: every row in every
// round; the same groups, the same rounds).
// Flow (query_pass.hpp): reconfigure(), complete_positions(), then per round and local a contiguous range of the active rows: upload,
// the launch (and the combine launch when the sources are split) on the local's compute stream, stream sync, copy back.  The rows are
// all N global rows whatever the context: in an nbody_init_rank job every rank walks them all on its own device and arrives at the same
// values; labels are not exchanged between processes.
// The pass reads pos[cur] and writes only the Local's fo_* buffers and q_scratch: positions, velocities, arrival counters, partial
// forces, the captured step graph and the force-kernel timer stay as they were.  Nothing outside this file refers to it.
#include "query_pass.hpp"
#include "fof_args.hpp"

#include <numeric>

using namespace nbg;

namespace nbi {

namespace {

// One round's link pass on local L over r.cnt active rows — entries [r.first, r.first + r.cnt) of `active` (uploaded), or with
// active == null the bodies of those indices themselves — against the labels `label` (uploaded), the m_i left in fo_min for the copy back
int launch_fof(Local& L, const int* label, const int* active, const Range& r, double b2) {
  HIPC(hipSetDevice(L.device));
  const size_t n = (size_t)g.n;
  NBC(L.fo_label.ensure(n * sizeof(int)));
  HIPC(hipMemcpy(L.fo_label, label, n * sizeof(int), hipMemcpyHostToDevice));
  if (active) {
    NBC(L.fo_rows.ensure((size_t)r.cnt * sizeof(int)));
    HIPC(hipMemcpy(L.fo_rows, active + r.first, (size_t)r.cnt * sizeof(int), hipMemcpyHostToDevice));
  }
  NBC(L.fo_min.ensure((size_t)r.cnt * sizeof(int)));
  const int n_blocks = source_blocks();
  const SplitPlan plan = chunk_split("NBODY_FOF_SPLIT", "NBODY_FOF_SCRATCH_MB", r.cnt, n_blocks, fof_scratch_bytes(1, 1));
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(fof_scratch_bytes((size_t)plan.batch, (size_t)plan.chunks)));
  return for_batches(r.cnt, plan, [&](int b0, int m) {
    FofArgs a;
    memset(&a, 0, sizeof(a));
    fill_sources(a, L, plan, n_blocks, m, active ? 0 : r.first + b0);
    a.label = L.fo_label.as<int>();
    a.rows = active ? L.fo_rows.as<int>() + b0 : nullptr;
    a.out = L.fo_min.as<int>() + b0;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<int>() : nullptr;
    a.b2 = b2;
    HIPC((hipError_t)nbl::launch_fof_kernel(g.fp64, L.compute, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_fof_combine_kernel(L.compute, a));
    return NBODY_OK;
  });
}

// the host's union-find: the root of a set is its lowest index
struct Sets {
  std::vector<int> parent;
  explicit Sets(int n) : parent((size_t)n) { std::iota(parent.begin(), parent.end(), 0); }
  int find(int i) {
    int r = i;
    while (parent[(size_t)r] != r) r = parent[(size_t)r];
    while (parent[(size_t)i] != r) { const int up = parent[(size_t)i]; parent[(size_t)i] = r; i = up; }
    return r;
  }
  void unite(int a, int b) {
    a = find(a); b = find(b);
    if (a < b) parent[(size_t)b] = a;
    else if (b < a) parent[(size_t)a] = b;
  }
};

// floor(log2 n) merging rounds and the silent last one: at most ceil(log2 n) + 1
int round_cap(int n) {
  int cap = 1;
  for (long long p = 1; p < n; p *= 2) ++cap;
  return cap;
}

int fof_impl(double b2, int* group, int* n_groups, int* rounds) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if ((!group && !n_groups) || !(b2 >= 0.0)) return NBODY_ERR_ARG;   // (a NaN b2 is not >= 0)
  NBC(reconfigure());
  NBC(complete_positions());
  const int n = g.n, cap = round_cap(n);
  const bool all_rows = env_ll("NBODY_FOF_ALL_ROWS", 0) == 1;
  const bool trace = env_ll("NBODY_FOF_TRACE", 0) == 1;   // a diagnostic, no part of include/nbody.h: a line per round on stderr (tools/fof_rate.py reads the rows walked from it)
  Sets sets(n);
  std::vector<int> label((size_t)n), active, found((size_t)n), next;
  std::vector<char> reported((size_t)n);
  std::iota(label.begin(), label.end(), 0);
  int done = 0;
  for (bool more = true; more;) {
    if (done == cap) return NBODY_ERR_STATE;
    const int* list = active.empty() ? nullptr : active.data();   // null: every row, the identity
    const int cnt = list ? (int)active.size() : n;
    NBC(run_on_locals([&](int l) { return points_of(cnt, l); },
                      [&](Local& L, const Range& r) { return launch_fof(L, label.data(), list, r, b2); },
                      [&](Local& L, const Range& r) { return copy_out(found.data(), r.out, L.fo_min, r.cnt, sizeof(int)); }));
    ++done;
    more = false;
    int told = 0;
    std::fill(reported.begin(), reported.end(), 0);
    for (int q = 0; q < cnt; ++q) {
      const int m = found[(size_t)q];
      if (m == kFoNone) continue;
      const int i = list ? list[q] : q;
      if (m < 0 || m >= n) return NBODY_ERR_STATE;   // no label the pass was given
      reported[(size_t)label[(size_t)i]] = 1;
      sets.unite(i, m);
      more = true;
      ++told;
    }
    if (trace) fprintf(stderr, "nbody_fof: round %d: %d rows, %d reported\n", done, cnt, told);
    if (!more) break;
    if (!all_rows) {   // the rows of the groups that reported, by their labels of this round, ascending
      next.clear();
      for (int q = 0; q < cnt; ++q) {
        const int i = list ? list[q] : q;
        if (reported[(size_t)label[(size_t)i]]) next.push_back(i);
      }
      active.swap(next);
    }
    for (int i = 0; i < n; ++i) label[(size_t)i] = sets.find(i);
  }
  if (group) memcpy(group, label.data(), (size_t)n * sizeof(int));
  if (n_groups) {
    int roots = 0;
    for (int i = 0; i < n; ++i) roots += label[(size_t)i] == i;
    *n_groups = roots;
  }
  if (rounds) *rounds = done;
  return NBODY_OK;
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_fof(float b2, int* group, int* n_groups, int* rounds) { NB_ENTER(0);
  return fof_impl((double)b2, group, n_groups, rounds);
}
int nbody_fof_d(double b2, int* group, int* n_groups, int* rounds) { NB_ENTER(1);
  return fof_impl(b2, group, n_groups, rounds);
}

}  // extern "C"
