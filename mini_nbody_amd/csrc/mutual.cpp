// mutual.cpp — the host side of the mutual pairing (NBODY_OPT_PAIRING, include/nbody.h): which force passes take it, the
// table of level-1 sums and the launch of mutual.hip.  Host C++ only.  A pass that does not take it is the ordered pass of
// context.cpp, untouched: nothing here changes ForceArgs, the kernel selection or the launch configuration.
#include "mutual_args.hpp"
#include "nbody_internal.hpp"

using namespace nbk;

namespace nbi {

namespace {

constexpr int kAutoRows = 1 << 20;   // AUTO takes the mutual pairing from here up (the XCD map's threshold: 4096 row blocks of 256)

// every piece of the ordered pass's segmentation (slices, segments, wave pieces) begins and ends on a block: a level-1 block then
// belongs to exactly one piece, and the sums of the fold (mutual.hip, fold_row) are the ordered pass's
bool whole_block_pieces(int n, const LaunchConfig& c) {
  for (int q = 0; q < c.nslices; ++q)
    for (int t = 0; t < c.sub; ++t) {
      int jb, je;
      segment_bounds(q, t, n, c.nslices, c.sub, &jb, &je);
      for (int w = 0; w < c.wsplit; ++w) {
        int pb = jb, pe = je;
        if (c.wsplit > 1) piece_bounds(jb, je, w, c.wsplit, &pb, &pe);
        if (pb % nbm::kBlock || pe % nbm::kBlock) return false;
      }
    }
  return true;
}

bool eligible(const Problem& p, int row0, int row_count, const Redirect* rd) {
  if (rd) return false;   // a mailbox request: its own sources, its own destination
  if (g.fp64 || g.opt.arith != NBODY_ARITH_FMA3 || g.opt.sum_order != NBODY_SUM_BLOCKED || g.opt.sum_block != nbm::kBlock || g.opt.masses) return false;
  if (g.nranks != 1 || g.nlocal != 1) return false;
  if (p.n != g.n || p.n_local != p.n || row0 != 0 || row_count != p.n) return false;
  if (p.n % nbm::kBlock || p.n > nbm::kMaxN) return false;
  return whole_block_pieces(p.n, p.cfg);
}

// *take: the pass runs in the mutual pairing, given a table
int choose(const Problem& p, int row0, int row_count, const Redirect* rd, bool* take) {
  *take = false;
  if (g.opt.pairing == NBODY_PAIRING_ORDERED) return NBODY_OK;
  const bool el = eligible(p, row0, row_count, rd);
  if (g.opt.pairing == NBODY_PAIRING_MUTUAL && !el) return NBODY_ERR_UNSUPPORTED;
  *take = el && (g.opt.pairing == NBODY_PAIRING_MUTUAL || row_count >= kAutoRows);
  return NBODY_OK;
}

inline size_t table_bytes(int n) { return (size_t)(n / nbm::kBlock) * (size_t)n * sizeof(f4); }

// the table of L for n bodies; *have = false: it could not be allocated (remembered: the passes run ordered)
int ensure_table(Local& L, int n, bool* have) {
  *have = false;
  if (g.mutual_no_table) return NBODY_OK;
  if (L.mutual_table && L.mutual_table.bytes >= table_bytes(n) && L.mutual_tickets) { *have = true; return NBODY_OK; }
  HIPC(hipSetDevice(L.device));
  bool moved = false;
  // the counters (one per row block, zero between passes) first: 4 KiB against the table's N^2 / 64 bytes
  if (L.mutual_tickets.ensure(((size_t)(n / nbm::kBlock) * sizeof(unsigned) + 255) / 256 * 256, true, &moved) != NBODY_OK ||
      L.mutual_table.ensure(table_bytes(n), false, &moved) != NBODY_OK) {
    (void)hipGetLastError();
    L.mutual_table.reset(); L.mutual_table.bytes = 0; L.mutual_tickets.reset(); L.mutual_tickets.bytes = 0;
    g.mutual_no_table = true;
    drop_step_graph();
    return NBODY_OK;
  }
  if (moved) drop_step_graph();   // captured launches hold the old table's address
  *have = true;
  return NBODY_OK;
}

}  // namespace

static int mutual_pass(const Problem& p, Local& L, int row0, int row_count, const Finish& fin, const Redirect* rd, bool* taken) {
  *taken = false;
  bool take = false;
  NBC(choose(p, row0, row_count, rd, &take));
  if (!take) return NBODY_OK;
  bool have = false;
  NBC(ensure_table(L, p.n, &have));
  if (!have) return NBODY_OK;
  HIPC(hipSetDevice(L.device));
  nbm::MutualArgs m;
  memset(&m, 0, sizeof(m));
  m.src = L.pos[L.cur];
  m.table = L.mutual_table.as<f4>();
  m.tickets = L.mutual_tickets.as<unsigned>();
  m.n = p.n; m.nb = p.n / nbm::kBlock;
  m.run = nbm::kRun;
  m.nunits = nbm::mutual_units(m.nb, m.run);
  ForceArgs& f = m.f;
  f.src = L.pos[L.cur]; f.rows = L.pos[L.cur];   // one rank: first_body = 0
  f.vel = L.vel;
  f.pos_next_rows = L.pos[L.cur ^ 1];
  f.force_out = fin.store_force ? (void*)L.force : nullptr;
  f.n_src = p.n; f.n_rows = p.n_local; f.row0 = 0; f.row_count = row_count;
  f.nslices = p.cfg.nslices; f.sub = p.cfg.sub; f.nseg = p.cfg.nseg; f.wsplit = p.cfg.wsplit;
  f.do_kick = fin.kick; f.do_drift = fin.drift;
  f.sum_block = nbm::kBlock;
  f.dt = fin.dt; f.dt64 = fin.dt64;
  int slot;
  NBC(timer_begin(L.kern, L.compute, &slot));
  HIPC((hipError_t)nbl::launch_mutual_pairs_kernel(L.compute, m));
  NBC(timer_end(L.kern, L.compute, slot));
  *taken = true;
  return NBODY_OK;
}

static int mutual_prepare_step() {
  if (!g.init || g.nlocal != 1) return g.opt.pairing == NBODY_PAIRING_MUTUAL ? NBODY_ERR_UNSUPPORTED : NBODY_OK;
  Local& L = g.loc[0];
  bool take = false, have = false;
  NBC(choose(problem_of(L), 0, L.n_local, nullptr, &take));
  if (take) NBC(ensure_table(L, g.n, &have));
  return NBODY_OK;
}

static int mutual_resolved_pairing() {
  if (!g.init || g.nlocal != 1) return NBODY_PAIRING_ORDERED;
  const Local& L = g.loc[0];
  bool take = false;
  if (choose(problem_of(L), 0, L.n_local, nullptr, &take) != NBODY_OK || !take) return NBODY_PAIRING_ORDERED;
  return g.mutual_no_table ? NBODY_PAIRING_NO_TABLE : NBODY_PAIRING_MUTUAL;
}

static void mutual_release() {
  for (int l = 0; l < kMaxLocal; ++l) {
    Local& L = g.loc[l];
    if (!L.mutual_table) continue;
    (void)hipSetDevice(L.device);
    L.mutual_table.reset(); L.mutual_table.bytes = 0;
    L.mutual_tickets.reset(); L.mutual_tickets.bytes = 0;
  }
  g.mutual_no_table = false;
}

// context.cpp reaches this file through g_mutual alone, so that it links without it (the host sanitizer harness's file lists)
static const MutualHooks kHooks = {mutual_pass, mutual_prepare_step, mutual_resolved_pairing, mutual_release};
static const bool kRegistered = (g_mutual = &kHooks, true);

}  // namespace nbi
