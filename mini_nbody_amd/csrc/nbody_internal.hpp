// nbody_internal.hpp — what the parts of libnbody_hip.so share (none of it crosses the C-ABI of include/nbody.h):
//   kernels.hip   the nbk kernels (nbody_kernels.hpp) and the thin launch functions that pick an instantiation (namespace nbl)
//   context.cpp   the context: options, launch configuration, buffers, the force pass (a function of the Problem it is given), the step
//                 and its HIP graph, state transfer, the strict gate
//   comm.cpp      RCCL (resolved with dlopen), the transfer plans, the all-gather of a step, probes and self-tests
//   mailbox.cpp   the reference's mailbox: RAM images, one request (a force pass over a Problem of the request's own N), the service thread
//   diag_pass.hpp  what the eight diagnostic passes below share on the device: the potential's pair arithmetic, the lane and wave
//                  preamble of a one-query-per-lane kernel, the block and workgroup sizes (read by their *_args.hpp)
//   query_pass.hpp what they share on the host: ranges over the locals, upload, the split's batches, launch-then-copy-back, the ranks' words
//   energy.hip    the energy pass's kernels (energy_args.hpp: its argument block and launch functions)
//   energy.cpp    nbody_energy, nbody_potential_rows(_d): the energy pass on every local and the sum over the ranks
//   point_sums.hip the field, tidal and jerk passes' kernels: one skeleton of blocked sums, a statement per pass (point_sums_args.hpp: the
//                  passes, their argument block and launch functions)
//   point_sums.cpp nbody_field(_d), nbody_tidal(_d): acceleration and potential, and the tidal tensor, at the caller's points, the
//                  points divided over the locals
//   neighbors.hip the neighbour pass's kernels (neighbors_args.hpp: its argument block and launch functions)
//   neighbors.cpp nbody_neighbors_rows(_d), nbody_nearest(_d), nbody_closest_pair(_d): nearest body, radius count, closest pair
//   knn.hip       the k-nearest-neighbour pass's kernels (knn_args.hpp: its argument block and launch functions)
//   knn.cpp       nbody_knn_rows(_d), nbody_knn(_d): the k nearest bodies of a row or a point and their squared distances
//   fof.hip       the friends-of-friends link pass's kernels (fof_args.hpp: its argument block and launch functions)
//   fof.cpp       nbody_fof(_d): the groups of a linking length, rounds of the link pass under a union-find on the host
//   hist.hip      the radial-count pass's kernels (hist_args.hpp: its argument block and launch functions)
//   hist.cpp      nbody_radial_counts_rows(_d), nbody_radial_counts(_d), nbody_pair_histogram(_d): bodies per shell of distance, pair counts
//   timescale.hip the pair time-scale pass's kernels (timescale_args.hpp: its argument block and launch functions)
//   timescale.cpp nbody_timescale_rows(_d), nbody_min_timescale(_d), nbody_step_adaptive(_d): pair crossing times, the shared adaptive step
//   pair_energy.hip the pair binding-energy pass's kernels (pair_energy_args.hpp: its argument block and launch functions)
//   pair_energy.cpp nbody_pair_energy_rows(_d), nbody_binaries: every body's most bound partner, the mutually most bound pairs and their elements
//   hermite.hip   the Hermite step's predictor, corrector and best-row reduction (hermite_args.hpp: their argument block and launch functions)
//   hermite.cpp   nbody_step_hermite(_d), nbody_min_aarseth, nbody_step_hermite_adaptive(_d): the fourth-order Hermite step on the jerk rows
//                 pass of point_sums.cpp, the smallest |a|^2 / |j|^2 of the system and the shared Aarseth time step
//                 (hermite_host.hpp: what it shares with hermite_block.cpp)
//   hermite_block.hip the block step's scheduler kernels: init, predict-to-tau, next-time, compact-and-gather, correct-and-assign
//                 (hermite_block_args.hpp: their argument block, the level rules and launch functions)
//   hermite_block.cpp nbody_step_hermite_block(_d): individual block time steps, the active rows evaluated by the jerk points pass
//   hermite6.hip  the sixth-order Hermite step's predictor and corrector with the crackle (hermite6_args.hpp: their argument block, the
//                 coefficients of a step and launch functions)
//   hermite6.cpp  nbody_step_hermite6(_d), nbody_step_hermite6_adaptive(_d): the sixth-order Hermite step on the snap rows pass
//   hermite6_block.hip the sixth-order block step's scheduler kernels: init, predict-to-tau, compact-and-gather, correct-and-assign
//                 (hermite6_block_args.hpp: their argument block and launch functions; the level rules and the next-time kernel are
//                 hermite_block_args.hpp's)
//   hermite6_block.cpp nbody_step_hermite6_block(_d): sixth-order individual block time steps, the active rows evaluated by the snap
//                 points pass
//   mutual.hip    the mutual pairing's kernel: every unordered pair of a full fp32 force pass once, the ordered pass's bits (mutual_args.hpp:
//                 its argument block, the unit enumeration and launch function)
//   mutual.cpp    which passes take the mutual pairing (NBODY_OPT_PAIRING), its table of level-1 sums and its launch
// Only kernels.hip, energy.hip, point_sums.hip, neighbors.hip, knn.hip, fof.hip, hist.hip, timescale.hip, pair_energy.hip, hermite.hip, hermite_block.hip, hermite6.hip, hermite6_block.hip and mutual.hip are device code (a minute of hipcc, as one code object through device.hip);
// the others are host C++ (seconds).  gfx950 only, no CPU fallback anywhere.
// Ownership: every stream, event, device and pinned allocation the context uses lives in an owning handle (Stream, Event, DevMem, Pinned,
// below) that is a member of Global or of one of its Locals; nbody_shutdown() releases them all, and nothing does at process exit (see `g`).
//
// Data layout in HBM (per rank; N bodies in total, the rank owns n_local of them starting at first_body):
//   pos[2]   2 x N words      full position set, double-buffered: a step reads pos[cur] and writes the
//                             rank's slice of pos[cur^1]; the other slices of pos[cur^1] arrive over xGMI
//   vel      n_local words    never leaves the rank in a step; the pair time-scale and jerk passes gather a copy of all N (ts_vel, full_scratch)
//   partial  nseg x rows'     per-source-segment partial forces (unused when nseg == 1); rows' = the launch's rows rounded up to 64
//   tickets  1 per 64 rows    arrival counters of the in-launch combine (zero between steps)
//   force    n_local words    last combined forces (parity entry points)
// word = {x,y,z,w}: 16 B (fp32) or 32 B (fp64) — the reference's RAM word, S/top_level.vhd:206-208.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only; the library is resolved with dlopen when nranks > 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/nbody.h"
#pragma GCC visibility pop
#include "nbody_args.hpp"

namespace nbi {

using nbk::ForceArgs;

// where the last HIP / RCCL error was seen (nbody_error_string); atomics: the mailbox's service thread may be the one that saw it
extern std::atomic<const char*> g_last_file;
extern std::atomic<int> g_last_line;
#define NB_MARK() do { ::nbi::g_last_file.store(__FILE__, std::memory_order_relaxed); ::nbi::g_last_line.store(__LINE__, std::memory_order_relaxed); } while (0)
// While nbody_mailbox_serve(1, .) is in effect the service thread owns the context: every entry point that launches, copies or
// reconfigures answers NBODY_ERR_STATE (nbody_get_info, nbody_error_string, nbody_mailbox_rams, nbody_mailbox_serve and nbody_shutdown do not)
#define NB_REFUSE_WHILE_SERVED() do { if (::nbi::mailbox_serving()) return NBODY_ERR_STATE; } while (0)
// ... and an entry point that exists in two precisions — is_d = 0: the float form, 1: the _d form — answers it on a context of the other
#define NB_ENTER(is_d) do { NB_REFUSE_WHILE_SERVED(); if (::nbi::g.init && (::nbi::g.fp64 != 0) != ((is_d) != 0)) return NBODY_ERR_STATE; } while (0)
// ... and an entry point whose physics is unit-mass answers NBODY_ERR_UNSUPPORTED while NBODY_OPT_MASSES is 1, after the two checks
// above and before anything is launched, copied or written: a refusal, never a silently unweighted answer
#define NB_REFUSE_MASSES() do { if (::nbi::g.opt.masses) return NBODY_ERR_UNSUPPORTED; } while (0)
#define NB_ENTER_UNIT_MASS(is_d) do { NB_ENTER(is_d); NB_REFUSE_MASSES(); } while (0)
#define HIPC(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { NB_MARK(); return (int)e_; } } while (0)
#define NBC(expr) do { int e_ = (expr); if (e_ != NBODY_OK) return e_; } while (0)
#define NCCLC(expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) { NB_MARK(); return 2000 + (int)r_; } } while (0)

constexpr int kMaxLocal = 16;
constexpr int kMaxRanks = 64;
constexpr int kTimerRing = 256;
constexpr int kGraphSteps = 32;    // steps per replayed HIP graph once a call brings at least twice as many

// ---- owning handles: one HIP resource each, move-only, released by reset(), by assignment over them or by their destructor ----
template <typename T, hipError_t (*Destroy)(T)>
struct Owned {
  T h = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
  Owned& operator=(Owned&& o) noexcept { std::swap(h, o.h); return *this; }   // (what this held goes with o)
  ~Owned() { reset(); }
  void reset() { if (h) { (void)Destroy(h); h = nullptr; } }
  T* put() { reset(); return &h; }   // for the HIP call that creates the resource
  operator T() const { return h; }
  template <typename U> U* as() const { return (U*)h; }   // memory: the typed pointer ForceArgs, EnergyArgs and RCCL calls take
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Graph = Owned<hipGraph_t, hipGraphDestroy>;   // scoped: a capture's graph until it is instantiated

// device memory (on the device that is current when it is allocated)
struct DevMem : Owned<void*, hipFree> {
  size_t bytes = 0;
  // at least `need` bytes: kept if large enough, else freed and allocated anew (*moved: the address is no longer what it was)
  int ensure(size_t need, bool zero = false, bool* moved = nullptr) {
    if (h && need <= bytes) return NBODY_OK;
    if (moved) *moved = true;
    reset(); bytes = 0;
    HIPC(hipMalloc(&h, need));
    bytes = need;
    if (zero) NBC(zero_now(h, need));
    return NBODY_OK;
  }
  // hipMemset of device memory does not wait for the fill, which runs on the null stream — and the context's streams are
  // hipStreamNonBlocking, so nothing they do later is ordered behind it: the zeros of nbody_init could land on an upload's copy.
  // The fill is drained before anything else may touch the buffer.
  static int zero_now(void* p, size_t bytes) {
    HIPC(hipMemset(p, 0, bytes));
    HIPC(hipStreamSynchronize(nullptr));
    return NBODY_OK;
  }
};
// pinned host memory; its users size it once per context, for the context's capacity
struct Pinned : Owned<void*, hipHostFree> {
  int ensure(size_t bytes, unsigned flags, bool zero = false) {
    if (h) return NBODY_OK;
    HIPC(hipHostMalloc(&h, bytes, flags));
    if (zero) memset(h, 0, bytes);
    return NBODY_OK;
  }
};

// a ring of HIP event pairs whose durations are summed lazily (no host sync while a step is being enqueued)
struct EventTimer {
  Event t0[kTimerRing], t1[kTimerRing];
  int head = 0, count = 0;
  double ms = 0.0;
  long long n = 0;
};

struct Local {
  int device = 0, rank = 0;
  int first = 0, n_local = 0;          // owned bodies
  Stream compute, comm;                // (declared first: destroyed after everything that ran on them)
  DevMem pos[2];
  DevMem vel;
  DevMem partial;                      // grown by ensure_partial
  DevMem tickets;                      // arrival counters (unsigned): one per 64 rows, see ticket_words()
  DevMem force;
  DevMem full_scratch;                 // N words: all-gather of a sharded array for the host (multi-process)
  DevMem en_part;                      // energy pass (energy.cpp): per-workgroup fp64 partials of {T, U, P, L} ...
  DevMem en_tot;                       // ... the ranks' totals, 8 doubles at word `rank` (all P after an all-gather) ...
  DevMem en_phi;                       // ... and phi of the rows asked for (context precision)
  DevMem q_points, q_skip;             // field, tidal, neighbour, knn and radial-count pass (query_pass.hpp): this local's range of the caller's points and skip indices ...
  DevMem q_scratch;                    // ... and what a launch whose sources are split leaves for its combine (point_sums_args.hpp, neighbors_args.hpp, knn_args.hpp, fof_args.hpp, hist_args.hpp, timescale_args.hpp)
  DevMem q_out[2];                     // field, tidal and jerk pass (point_sums.cpp): the points' outputs (context precision), shared as q_points is
  DevMem q_vel;                        // jerk pass (point_sums.cpp): this local's range of the caller's point velocities
  DevMem q_acc, q_out2;                // snap pass (point_sums.cpp): this local's range of the caller's point accelerations, and the third output ...
  DevMem sn_acc, sn_acc_all;           // ... the own rows' accelerations of the jerk rows pass a snap call opens with (n_local words), and all N acceleration words where the snap kernel reads them (query_pass.hpp, gather_accelerations)
  DevMem nb_idx, nb_d2, nb_count;      // neighbour pass (neighbors.cpp): the queries' outputs (d2 in the context precision) ...
  DevMem nb_best;                      // ... and the ranks' closest pairs, one BestPair at word `rank` (all P after an all-gather)
  DevMem kn_idx, kn_d2;                // knn pass (knn.cpp): the queries' outputs, k entries each (d2 in the context precision)
  DevMem hi_count;                     // radial-count pass (hist.cpp): the queries' counts, n_bins each ...
  DevMem hi_sums;                      // ... and the ranks' pair-histogram sums, NBODY_HIST_MAX_BINS 64-bit sums at word `rank` (all P after an all-gather)
  DevMem ts_vel;                       // pair time-scale and jerk pass (query_pass.hpp, gather_velocities): all N velocity words, gathered at the start of a call (several devices in one process) ...
  DevMem ts_tau2, ts_idx, ts_d2;       // ... the rows' outputs (tau2 and d2min in the context precision) ...
  DevMem ts_best;                      // ... and the ranks' bests, one BestScale at word `rank` (all P after an all-gather)
  DevMem pe_e, pe_idx;                 // pair binding-energy pass (pair_energy.cpp): the rows' outputs (e in the context precision)
  DevMem fo_label, fo_rows, fo_min;    // fof pass (fof.cpp): the N labels of a round, this local's range of the active rows and their m_i
  DevMem he_pos0, he_vel0;             // Hermite step (hermite.cpp): the own rows' (x0, v0) of the step under way, n_local words each ...
  DevMem he_acc[2], he_jerk[2];        // ... their acceleration and jerk words at the start of the step and at the predicted state ...
  DevMem he_best;                      // ... and the ranks' smallest |a|^2 / |j|^2, one BestRatio at word `rank` (all P after an all-gather)
  DevMem h6_snap[2], h6_crk, h6_ap;    // sixth-order Hermite step (hermite6.cpp): the own rows' snap words at both ends of the step, the crackle the next predictor takes and the predicted accelerations; the rest is he_pos0, he_vel0, he_acc, he_jerk, he_best
  DevMem hb_tick, hb_level;            // block time steps (hermite_block.cpp): the own rows' ticks (64-bit) and levels; their base is he_pos0, he_vel0, he_acc[0], he_jerk[0] ...
  DevMem hb_counts, hb_active;         // ... the active rows of a sub-step per tile of 256 rows and their ascending list (their queries go to q_points, q_vel, q_skip) ...
  DevMem hb_next;                      // ... and the ranks' next times, one NextTime at word `rank` (all P after an all-gather)
                                       // sixth-order block time steps (hermite6_block.cpp): hb_* as above; the base is he_pos0, he_vel0, he_acc[0], he_jerk[0], h6_snap[0], h6_crk; he_acc[1], he_jerk[1], h6_snap[1] take the active rows' evaluations, h6_ap every own row's predicted acceleration, q_acc the queries' (no buffer of its own)
  DevMem mutual_table;                 // mutual pairing (mutual.cpp): the level-1 sums T[source block][row], N / 1024 x N words; allocated when a pass first takes that path ...
  DevMem mutual_tickets;               // ... and its counters, one per row block: table words written so far (zero between passes)
  int cur = 0;
  bool all_present = true;             // pos[cur] holds every slice
  Event ev_own_ready;                  // the rank's slice of pos[cur] is written
  Event ev_comm_go;                    // the transfer stream has seen ev_own_ready: its RCCL kernel is next on its queue
  Event ev_gather[kMaxRanks];
  ncclComm_t comm_h = nullptr;
  EventTimer kern;   // force kernels (NBODY_OPT_TIMING)
  EventTimer wait;   // how long the compute stream sat waiting for arriving slices: exposed communication
};

struct Options {
  int variant = NBODY_VARIANT_AUTO, iblock = 0, jsub = 0, jslices = 0;
  int arith = NBODY_ARITH_FMA3, sum_order = NBODY_SUM_BLOCKED, sum_block = 1024, fuse = -1;
  int timing = 0, comm = NBODY_COMM_AUTO, overlap = 1, isa_phase = 1, waves_per_simd = 0, graph = 1, long_buffers = -1, xcd_map = -1;
  int wsplit = -1;
  int pairing = NBODY_PAIRING_AUTO;   // NBODY_OPT_PAIRING: which full fp32 force passes evaluate every unordered pair once (mutual.cpp)
  int masses = 0;   // NBODY_OPT_MASSES: the ordered-sum passes weigh source j by the w of its position word (a launch argument, no state)
};

// what happens to the force of a row once all its segments are summed, and the time step of a kick or drift
struct Finish { bool kick, drift, store_force; float dt = 0.f; double dt64 = 0.0; };

// what one launch reads and writes instead of the context's buffers (a mailbox request); none by default
struct Redirect {
  void* force_dst = nullptr;                // {Fx,Fy,Fz,0} stored here instead of Local::force (RAM B itself)
  const void* src_direct = nullptr;         // sources and rows read from here instead of pos[cur] (RAM A itself: no ingest launch) ...
  unsigned long long* t0_stamp = nullptr;   // ... and the 16-row kernel's first wave stamps the tick count's start here (ForceArgs::t0_stamp)
};

// the resolved launch configuration: what resolve_config() makes of N, the rank count, precision, options and CU count
struct LaunchConfig {
  int variant = NBODY_VARIANT_SMEM, R = 4, sub = 1, nslices = 1, nseg = 1, fuse = 1;
  int wsplit = 1;                 // 4: a workgroup owns 64 rows, its four waves walk a quarter of the segment each (ForceArgs::wsplit)
  bool operator==(const LaunchConfig& o) const {
    return variant == o.variant && R == o.R && sub == o.sub && nslices == o.nslices && nseg == o.nseg && fuse == o.fuse && wsplit == o.wsplit;
  }
  bool operator!=(const LaunchConfig& o) const { return !(*this == o); }
};

// What a force pass works on: n sources, a local that owns n_local rows of them, and the launch configuration resolved for that.  The
// context's own passes take {g.n, L.n_local, g.cfg} (problem_of); a mailbox request makes one of its NUM_PTS and touches none of the three.
struct Problem { int n = 0, n_local = 0; LaunchConfig cfg; };

typedef int (*host_gather_fn)(void* user, void* host_words, int n_total, int word_bytes, int rank, int nranks);

struct Global {
  host_gather_fn host_gather = nullptr;   // multi-process fallback transport: slices exchanged through host memory
  void* host_gather_user = nullptr;
  Pinned host_stage;                      // staging buffer, N words
  // the mailbox's two RAMs as the PS sees them (mailbox.cpp: mailbox_rams), its completion word, and the device-side start stamp
  struct MailboxMem { Pinned a, b, seq; DevMem t0; } mb;
  // HIP graph of an even number of consecutive steps (the position buffers swap every step, so a pair returns to the same state):
  // replayed by nbody_step when one GPU runs many short steps (launch-bound regime)
  hipGraphExec_t step_graph = nullptr;
  bool stepped_eagerly = false;   // a step has been launched outside a capture since nbody_init
  float graph_dt = 0.f; double graph_dt64 = 0.0; int graph_cur = -1, graph_len = 0;
  bool init = false;
  int n = 0, fp64 = 0, tile = 256;
  int cap = 0;                    // body words the buffers were allocated for (= the n of nbody_init; a mailbox request may bring fewer)
  int nranks = 1, nlocal = 0;
  bool multiprocess = false;
  Local loc[kMaxLocal];
  Options opt;
  LaunchConfig cfg;
  bool comm_go_armed = false;     // the gather just enqueued recorded ev_comm_go (RCCL transport)
  bool mutual_no_table = false;   // the mutual pairing's table could not be allocated: its passes run ordered (NBODY_INFO_PAIRING says so) until NBODY_OPT_PAIRING is set again
  bool tickets_dirty = false;     // a launch sequence failed part-way (TicketGuard): the arrival counters may be non-zero
  int cu_count = 0, clock_khz = 0;
  int comm_priority = 0;          // HIP priority of the transfer streams (0 = default)
  long long steps_done = 0;
};
// Who writes what: n in init_common, Local::n_local in describe_local, cfg in reconfigure() — none of them while the mailbox's service
// thread runs (NB_REFUSE_WHILE_SERVED), and a mailbox request writes none of them: nbody_get_info may read all three from any thread.
// The context is never destroyed: it is allocated once and its handles are released by nbody_shutdown() alone.  A process that exits
// without nbody_shutdown() therefore frees nothing and makes no HIP call after main() returns (static destructors may run after the HIP
// runtime's own teardown).
extern Global& g;

// nbody_shutdown() on every way out of opening a context (nbody_init, nbody_init_rank, nbody_mailbox_open) that is not commit()
struct OpenGuard {
  bool committed = false;
  int commit() { committed = true; return NBODY_OK; }
  ~OpenGuard() { if (!committed) nbody_shutdown(); }
};

inline size_t word_bytes() { return g.fp64 ? 32 : 16; }
inline char* word_ptr(void* base, size_t word) { return (char*)base + word * word_bytes(); }
inline int ring_slice(int rank, int s) { int q = (rank - s) % g.nranks; return q < 0 ? q + g.nranks : q; }
// arrival counters: one per 64 rows (a wave's rows), with slack for the row blocks of 256*R rows whose waves count in
// strides of 4*R, padded to a multiple of 256 bytes
inline size_t ticket_words(int n_local) { return ((size_t)(n_local + 63) / 64 + 32 + 63) / 64 * 64; }

// A sequence of force launches that fails part-way leaves arrival counters at a partial count: the next launch would combine early.
// Every caller of such a sequence (a step, forces_on_device, bodyForce, the comm probe, a mailbox request up to its completion) holds
// a TicketGuard around it; any way out before done() marks the counters dirty, and the next upload, reconfigure() or mailbox request re-zeroes
// them (zero_tickets) before it launches anything.
struct TicketGuard {
  bool ok = false;
  int done() { ok = true; return NBODY_OK; }
  ~TicketGuard();
};

// A window of rows as nbody_forces_rows and nbody_potential_rows take it — nbody_init contexts: GLOBAL body index, the range may span
// devices; nbody_init_rank contexts: row of this rank's own slice — held as the global bodies [g0, g0 + count) (count < 0: all N)
struct RowWindow {
  int g0 = 0, count = -1;
  int open(int first_row, int n_rows);                   // NBODY_ERR_ARG: not a non-empty range of the context's rows
  bool rows_of(const Local& L, int* r0, int* n) const;   // rows [*r0, *r0 + *n) of L's slice are in the window; false: none are
};

// ---- context.cpp ----
LaunchConfig resolve_config(int n, int nranks, int fp64, const Options& opt, int cu_count);
int reconfigure();
int ensure_partial(Local& L, int rows, int nseg);   // partial sums for nseg segments of a launch of `rows` rows on L
int zero_tickets();                       // every local's arrival counters, and the dirty mark off (TicketGuard sets it)
void drop_step_graph();
int timer_begin(EventTimer& T, hipStream_t stream, int* slot);
int timer_end(EventTimer& T, hipStream_t stream, int slot);
int timer_drain(EventTimer& T, int keep);
inline Problem problem_of(const Local& L) { return {g.n, L.n_local, g.cfg}; }   // the context's own problem on local L
// the force kernel of problem p on local L for rows [row0, row0 + row_count) against `nsl` source slices starting at slice_start and descending
int launch_force(const Problem& p, Local& L, int row0, int row_count, int slice_start, int nsl, const Finish& fin, const Redirect* rd = nullptr);
int launch_combine(const Problem& p, Local& L, int row0, int row_count, const Finish& fin, const Redirect* rd = nullptr);
// one whole force pass: launch_force over all of p's slices, then launch_combine
int force_pass(const Problem& p, Local& L, int row0, int row_count, const Finish& fin, const Redirect* rd = nullptr);
// launch_force would take the 16-row FPGA kernel (force_fpga16r_f32) for a launch of row_count rows in configuration cfg
bool takes_rows16(const LaunchConfig& cfg, int row_count);
int sync_all();
int complete_positions();
int step_impl(float dt, double dt64, int nsteps);   // nbody_step(_d): nsteps steps of dt (dt64 in an fp64 context); fewer than 4 are launched eagerly
int forces_impl(const void* pos_words, void* force_words, int n);
int device_count(int* ndev);
int pick_device(int rank, int ndev);

// ---- mutual.cpp: the mutual pairing of a full fp32 force pass (mutual_args.hpp), reached through g_mutual ----
struct MutualHooks {
  // The pass of problem p on L over rows [row0, row0 + row_count) in the mutual pairing, if NBODY_OPT_PAIRING and the pass's eligibility say
  // so: *taken = true and its launch is enqueued (one timed span); *taken = false: the caller runs the ordered pass.  NBODY_ERR_UNSUPPORTED,
  // nothing launched: NBODY_PAIRING_MUTUAL is forced and the pass is not eligible.
  int (*pass)(const Problem& p, Local& L, int row0, int row_count, const Finish& fin, const Redirect* rd, bool* taken);
  int (*prepare_step)();        // before a step is enqueued or captured: the refusal above, and the table allocated outside any capture
  int (*resolved_pairing)();    // NBODY_INFO_PAIRING: what a step of the context takes
  void (*release)();            // the tables freed (NBODY_OPT_PAIRING set: the next mutual pass allocates anew)
};
// mutual.cpp's functions once it is linked (the library: always); null in a program built from context.cpp without it, where every pass is
// ordered and NBODY_PAIRING_MUTUAL is refused
extern const MutualHooks* g_mutual;

// ---- comm.cpp ----
int rccl_load();
int comm_create(Local& L, int nranks, int rank, const void* uid128);   // ncclCommInitRank on L.device
void comm_destroy(Local& L);
int resolved_comm_form();
int enqueue_gather(int buf);                                    // bring the other ranks' slices of pos[buf] to every local
int gather_sharded_multiprocess(Local& L, const void* own_rows);   // a rank-sharded array into L.full_scratch
// word `rank` of dev_words (word_bytes each, written on the compute stream) of every rank into host_words[0 .. P) on every rank
int allgather_rank_words(Local& L, void* dev_words, void* host_words, int word_bytes);

// ---- mailbox.cpp ----
void mailbox_shutdown();          // stops the service thread, frees the RAM images
bool mailbox_serving();           // nbody_mailbox_serve(1, .) is in effect
long long mailbox_served();       // requests the service thread has completed in this process

}  // namespace nbi

// ---- kernels.hip: every kernel launch of the library ----
namespace nbl {
// which instantiation of the force kernel a launch takes (the rest travels in ForceArgs: wsplit, fpga16, long_buffers)
struct KernelSel {
  int fp64, variant, R, arith, tile, isa_phase;
  int fpga_lds;     // the FPGA order on sixteen waves: 1 = sources staged through LDS (default), 0 = scalar delivery (NBODY_VARIANT_SMEM asked for)
  int fpga_rows16;  // the FPGA order, one segment, a small launch: 16 rows x 16 chains per 256-thread workgroup (grid.x = 16-row units)
  size_t dyn_lds;   // dynamic LDS per workgroup: the occupancy cap of NBODY_OPT_WAVES_PER_SIMD (0 = none)
};
// all return a hipError_t as int (0 = launched)
int launch_force_kernel(const KernelSel& k, hipStream_t stream, dim3 grid, const nbk::ForceArgs& a);
int launch_combine_kernel(int fp64, hipStream_t stream, dim3 grid, const nbk::ForceArgs& a);
int launch_drift_kernel(int fp64, hipStream_t stream, void* pos_rows, const void* vel, int n_rows, float dt, double dt64);
int launch_ingest_kernel(hipStream_t stream, void* dst_words, const void* ram_a_bodies, int n, unsigned long long* t0);
int launch_mailbox_done_kernel(hipStream_t stream, void* word0, unsigned* seq_word, const unsigned long long* t0, unsigned seq,
                               unsigned clock_khz, unsigned rt_khz);
int launch_rsqrt_selftest_kernel(unsigned first_bits, unsigned long long count, unsigned long long* out3);
int launch_rsqrt_array_kernel(const float* x, float* y, int n, int ieee_only);
bool diag_build();   // this is libnbody_hip_diag.so (-DNBODY_DIAG_LOOPS): experiment encodings and timing-only loop forms present
}  // namespace nbl
