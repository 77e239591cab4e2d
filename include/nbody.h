/* nbody.h — C-ABI of the MI355X all-pairs N-body engine (libnbody_hip.so).
 *
 * Plain C99: pointers, ints, floats.  No HIP, torch or C++ types cross this
 * boundary.  The library behind it is hand-written HIP for gfx950
 * (mini_nbody_amd/csrc/: kernels.hip, energy.hip, point_sums.hip, neighbors.hip, knn.hip, fof.hip, hist.hip, timescale.hip, pair_energy.hip, hermite.hip, hermite_block.hip, hermite6.hip, hermite6_block.hip, mutual.hip + context.cpp, comm.cpp, mailbox.cpp, energy.cpp, point_sums.cpp, neighbors.cpp, knn.cpp, fof.cpp, hist.cpp, timescale.cpp, pair_energy.cpp, hermite.cpp, hermite_block.cpp, hermite6.cpp, hermite6_block.cpp, mutual.cpp); there is
 * no CPU fallback: every entry
 * point fails with NBODY_ERR_NO_DEVICE when no GPU is usable.
 *
 * WHAT EACH ENTRY POINT REPLACES.  The reference (/root/reference, a VHDL FPGA
 * design; "S/" = vec_add.srcs/sources_1/new/) has no function ABI: its only
 * boundary is a memory-mapped mailbox:
 *   - bodies in:  128-bit words {x, y, z, ignored} at word k = 1..N of RAM A    S/top_level.vhd:206-208, 238-240, 280
 *   - start:      word 0 = {bit 0 BEGIN, bits 46:32 NUM_PTS}                   S/top_level.vhd:184-185
 *   - forces out: 128-bit words {Fx, Fy, Fz, 0}: body k's at word k of RAM B,  S/compute_store.vhd:213, 221-242
 *                 word 0 never written
 *   - done:       word 0 rewritten with {ticks in bits 63:32}, BEGIN reads 0   S/top_level.vhd:146, 255-263
 *   - one request in flight; BEGIN ignored while busy                          S/top_level.vhd:180-186
 * The names bodyForce()/integrate() and the {pos, vel} layout come from
 * BASELINE.json's north_star (the host program they would belong to is not in
 * the reference tree); the 16-byte body word is the reference's.
 *
 * Conventions: every function returns 0 (NBODY_OK) on success; a positive value
 * < 1000 is a hipError_t, 1000..1999 an NBODY_ERR_*, 2000 + r an ncclResult_t r.
 * The caller owns host buffers, the library owns device buffers.  One context
 * per process, not thread-safe (the reference's single in-flight request); the one second thread the library knows — the mailbox's
 * service thread — locks every other caller out while it serves (nbody_mailbox_serve).
 */
#ifndef NBODY_H
#define NBODY_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBODY_OK 0
#define NBODY_ERR_NOT_INIT 1001
#define NBODY_ERR_ARG 1002
#define NBODY_ERR_NO_DEVICE 1003
#define NBODY_ERR_RCCL_LOAD 1004
#define NBODY_ERR_STATE 1005
#define NBODY_ERR_UNSUPPORTED 1006

/* Structure of arrays: two arrays of N 16-byte words.
 * pos[4i..4i+3] = {x, y, z, w}   (w is carried, never read by the force: S/top_level.vhd:206-208 ignores bits 127:96)
 * vel[4i..4i+3] = {vx, vy, vz, 0} */
typedef struct { float *pos, *vel; } BodySystem;
typedef struct { double *pos, *vel; } BodySystemD; /* fp64 configuration: N x 4 doubles (32-byte words) */

/* ---- options (nbody_set_option; all have working defaults) ---- */
enum {
  NBODY_OPT_VARIANT = 1,   /* how source bodies reach the lanes: NBODY_VARIANT_* */
  NBODY_OPT_IBLOCK = 2,    /* bodies per lane (register blocking) 1, 2, 4 or 8; 0 = auto */
  NBODY_OPT_JSUB = 3,      /* sub-segments per source slice; 0 = auto */
  NBODY_OPT_JSLICES = 4,   /* single-GPU only: number of source slices (to reproduce a P-GPU summation order bit for bit) */
  NBODY_OPT_ARITH = 5,     /* NBODY_ARITH_* */
  NBODY_OPT_SUM_ORDER = 6, /* NBODY_SUM_* */
  NBODY_OPT_TIMING = 7,    /* 1: HIP events around every force kernel (nbody_kernel_time) */
  NBODY_OPT_COMM = 8,      /* NBODY_COMM_* (multi-GPU) */
  NBODY_OPT_OVERLAP = 9,   /* multi-GPU: 1 = start on the rank's own slice while the others travel, then one launch over the
                              arrived slices (default); 2 = one launch per arriving slice, each released by that slice's
                              event; 0 = gather first, one launch */
  NBODY_OPT_SUM_BLOCK = 13, /* NBODY_SUM_BLOCKED: sources per level-1 block (multiple of 64; default 1024) */
  NBODY_OPT_XCD_MAP = 16,  /* 1: workgroups that share an XCD take the same source segments (launches with a multiple of 8 segment
                              rows), so each XCD's L2 fetches its segments once; 0: (blockIdx.x, blockIdx.y) = (row block, segment);
                              -1 (default): on for launches of >= 4096 row blocks (N = 1M: -39 % memory-side traffic at level time;
                              smaller launches measured slower with it).  Same results either way. */
  NBODY_OPT_ISA_LONG_BUFFERS = 15, /* NBODY_VARIANT_ISA: scalar buffers of 8 bodies instead of 4 (-1 = auto: when a launch has fewer
                              than 32 workgroups per CU; 0, 1 = force).  Same bits either way. */
  NBODY_OPT_FUSE_COMBINE = 14, /* 1: the segments' partial sums are added by the last wave to arrive, inside the force launch (one
                              launch per step); 0: a separate combine kernel; -1 (default): one launch when the launch has
                              >= 4 workgroups per CU, where the hand-off hides behind other workgroups, else two.  Same bits. */
  NBODY_OPT_GRAPH = 12,    /* nbody_step on one GPU replays a captured HIP graph of an even number of steps: 1 (default) = 32 steps per graph
                              when the call brings >= 64 (after the engine's first, eagerly launched step), 16 from 32, 8 from 16, else 2;
                              k >= 2 = k steps per graph (rounded down to even); 0: launch every kernel.  Same bits in every case. */
  NBODY_OPT_WAVES_PER_SIMD = 11, /* cap the force kernel's occupancy at k waves per SIMD (0 = no cap): tuning knob */
  NBODY_OPT_WSPLIT = 17,   /* 4 / 16: a workgroup owns 64 bodies and its 4 / 16 waves walk one piece of the source segment each; the
                              sums are added through LDS in ascending source order (a third level of the sum, like the reference's
                              16 partial sums + adder tree, S/fxyz.vhd:129-145, S/final_adder.vhd:88-104).  Same number of waves and
                              walk per wave from a quarter / a sixteenth of the global partial sums.  1: a workgroup owns
                              256 x IBLOCK bodies, every wave walks the whole segment (round 2's layout; the LDS / READLANE
                              kernels always).  -1 (default): where the kernel has it (SMEM and ISA deliveries, one body per lane),
                              16 when a rank owns <= 8192 bodies (fp32), else 4; 1 with NBODY_SUM_SEQ in fp32, which means ONE
                              sequential sum per segment.
                              With NBODY_SUM_FPGA16 (fp32) the split is of another kind and changes NO bit: -1 / 4 / 16 put the
                              reference's sixteen partial sums of a body on the sixteen waves of a workgroup (wave k walks the
                              sources k, k + 16, ... of the segment; wave 0 adds rotation and tree), 1 keeps all sixteen in one lane
                              (rounds 1-3).  Sixteen times the waves: the mailbox's maximum N = 32767 takes 0.51 ms per pass
                              instead of 2.56 (NBODY_INFO_WSPLIT then reports 16).  Round 6, still the same bits: the sixteen-wave form
                              stages its sources through LDS (NBODY_OPT_VARIANT = NBODY_VARIANT_SMEM keeps round 4's scalar delivery),
                              and a ONE-segment launch of fewer than 64 x CUs rows — the mailbox's faithful mode below N = 16384 — gives a
                              256-thread workgroup 16 rows x 16 partial sums, one (row, partial sum) per lane: four times the workgroups
                              where 64 rows per workgroup would leave CUs idle (N = 1024: 16 workgroups -> 64; NBODY_INFO_WSPLIT still
                              reports 16: sixteen partial sums per row, side by side). */
  NBODY_OPT_MASSES = 18,   /* 0 (default): unit masses, the w of a position word is carried and never read.  1: body j has the mass
                              m_j = the w of its position word AS IT LIES ON THE DEVICE, in the context precision — no separate array:
                              uploaded with the positions, downloaded with them, carried bit for bit by every integrator and every
                              gather.  The ordered-sum passes (energy and potential, field, tidal tensor, jerk) then weigh source j by
                              m_j, one more rounding per pair ("with NBODY_OPT_MASSES" in each section below), and the Hermite
                              integrators inherit it from the jerk; the distance passes and the pair time scale are geometry and
                              kinematics and do not change.  The entry points whose physics is unit-mass — bodyForce(_d),
                              nbody_step(_d), nbody_forces(_d), nbody_forces_rows(_d), nbody_step_adaptive(_d),
                              nbody_pair_energy_rows(_d), nbody_binaries, nbody_mailbox_run, nbody_mailbox_serve(1, .) — answer
                              NBODY_ERR_UNSUPPORTED while it is 1, before anything is launched, copied or written.  Setting it
                              launches nothing and invalidates nothing: the captured step graph, the arrival counters and the timers
                              stay.  With 0 every entry point returns the bits it returned without the option.  Any other value:
                              NBODY_ERR_ARG.  DOMAIN: queries have no mass (the w of a `points` word is ignored); a NaN mass poisons
                              every query that does not skip the body; an infinite mass gives +-inf or NaN; negative masses are
                              computed as written and nothing is promised about them.  Three exact properties: with every w = 1
                              the weighted form has the unweighted form's bits; multiplying every w by 2^k multiplies every output
                              by 2^k exactly (short of overflow and subnormals); a body with w = +0 at a finite position leaves
                              every sum it enters as it was, so massless bodies appended behind the massive ones change no bit of
                              the massive rows' results and are themselves accelerated (tracers). */
  NBODY_OPT_PAIRING = 19,  /* NBODY_PAIRING_*: how a FULL fp32 force pass (nbody_step, nbody_forces, bodyForce, nbody_forces_rows over all
                              rows) walks its pairs.  ORDERED: every row walks every source (each unordered pair evaluated twice).  MUTUAL:
                              every unordered pair is evaluated once and feeds both rows — still one launch: the kernel leaves the
                              level-1 sums of every (row, 1024-source block) in a table of N / 1024 x N 16-byte words (16 GiB at N = 2^20,
                              allocated when a pass first takes this path), and the wave that writes the last word of a block of 1024 rows
                              adds that block's sums in the ordered pass's own order:
                              THE SAME BITS as ORDERED in the same configuration, except that a NaN may differ in sign and payload (the
                              set of non-finite output words is the same).  Eligible: fp32, NBODY_ARITH_FMA3, NBODY_SUM_BLOCKED with
                              NBODY_OPT_SUM_BLOCK 1024, unit masses, one rank on one device, all rows, N a multiple of 1024 and every piece
                              boundary of the resolved segmentation (slices, segments, wave pieces) a multiple of 1024.  MUTUAL on a pass
                              that is not eligible: NBODY_ERR_UNSUPPORTED before anything is launched.  AUTO (default): MUTUAL for
                              eligible passes of >= 1048576 rows, else ORDERED.  If the table cannot be allocated the pass runs ORDERED and
                              NBODY_INFO_PAIRING says so. */
  NBODY_OPT_ISA_PHASE = 10 /* NBODY_VARIANT_ISA: which generated form of the hand-scheduled loop runs (tools/gen_force_loop.py).
                              1 = the product loop (default); 0 = the same instructions placed one 4-byte phase off (-27 %, kept
                              so that the placement effect can be re-measured).  fp64: 1 = the product loop (VALU instructions at
                              0 mod 8 bytes), 0 = one phase off (-1.2 %), 2 = eps and 3/8 from VGPR pairs (-0.9 %).
                              Every other value (fp32 2..18: experiment encodings of the same operations, and TIMING-ONLY forms
                              WITH WRONG RESULTS that price one part of the loop, profiles/r02_loop_diagnostics.md) exists only in
                              the diagnostic build `make diag` (libnbody_hip_diag.so, -DNBODY_DIAG_LOOPS); this library answers
                              NBODY_ERR_UNSUPPORTED. */
};
enum { NBODY_VARIANT_AUTO = 0,     /* ISA for the timed arithmetic (fp32, FMA3, blocked or sequential sum), else SMEM */
       NBODY_VARIANT_SMEM = 1,     /* wave-uniform scalar loads (s_load_dwordx16) into SGPRs: no LDS, no VALU cost */
       NBODY_VARIANT_LDS = 2,      /* `tile` bodies staged in LDS per workgroup, broadcast ds_read_b128 */
       NBODY_VARIANT_READLANE = 3, /* 64-body wave tile in VGPRs, v_readlane broadcast ("__shfl") */
       NBODY_VARIANT_ISA = 4       /* SMEM delivery with the inner loop hand-scheduled in gfx950 ISA (uniform 64-bit encodings,
                                      parity-safe registers); one body per lane, NBODY_ARITH_FMA3 only */ };
enum { NBODY_ARITH_FMA3 = 0,       /* d2 = fma(dx,dx,fma(dy,dy,fma(dz,dz,eps))): 11 VALU + v_rsq_f32 per pair.  THE TIMED MODE */
       NBODY_ARITH_REFERENCE = 1,  /* d2 = (dx*dx+dy*dy)+fma(dz,dz,eps): the RTL's rounding points, S/dxy.vhd:113-122, S/dzsoft.vhd:201-202, S/dxyz_soft.vhd:149-150 */
       NBODY_ARITH_STRICT = 2,     /* FMA3 with 1/sqrt rounded once from an fp64 evaluation instead of v_rsq_f32 (1 ulp):
                                      every operation is then IEEE-exact and the result is bit-identical to the CPU oracle.
                                      In an fp64 context: 1/sqrt as IEEE sqrt and divide instead of v_rsq_f64 + one third-order
                                      step — bit-identical to the oracle's fp64 evaluation in the configured summation order.
                                      DOMAIN of the timed fp64 FORCE (NBODY_ARITH_FMA3 in an fp64 context: bodyForce_d, nbody_step_d,
                                      nbody_forces_d, nbody_forces_rows_d): the squares of the coordinate differences must not overflow
                                      binary64 (|difference| below about 1.3e154).  Beyond that d2 = +inf, the seed is 0, the step's
                                      e = fma(-inf, 0, 1) is NaN and the pair contributes NaN, to every row that sees it, where
                                      NBODY_ARITH_STRICT contributes exactly +0: NBODY_ARITH_STRICT has no such limit.  The fp32 timed
                                      mode has none either (v_rsq_f32(inf) = 0, inv3 = 0), nor have the fp64 diagnostic passes below
                                      (energy, potential, field), which return the seed when it is 0. */
       NBODY_ARITH_REFERENCE_STRICT = 3 /* REFERENCE roundings + strict 1/sqrt (fp64 contexts have ONE d2 form — the fma-contracted one,
                                           as the oracle's fp64 evaluation — so there REFERENCE = FMA3 and REFERENCE_STRICT = STRICT) */ };
enum { NBODY_SUM_SEQ = 0,          /* one accumulator per segment, sources ascending (S/top_level.vhd:233-254) */
       NBODY_SUM_FPGA16 = 1,       /* 16 interleaved partials + pairwise tree (S/fxyz.vhd:129-184, S/final_adder.vhd:88-104) */
       NBODY_SUM_BLOCKED = 2       /* fp32 DEFAULT, THE TIMED MODE: two levels — blocks of NBODY_OPT_SUM_BLOCK consecutive sources
                                      are summed from zero, the block sums are added in ascending order.  The reference keeps
                                      16 partial sums + an adder tree for the same reason (S/fxyz.vhd:129-145,
                                      S/final_adder.vhd:88-104): one fp32 accumulator over 2^20 terms is off by 1e-4.
                                      fp64 contexts always sum sequentially. */ };
enum { NBODY_PAIRING_AUTO = 0, NBODY_PAIRING_ORDERED = 1, NBODY_PAIRING_MUTUAL = 2,
       NBODY_PAIRING_NO_TABLE = 3 /* a value of NBODY_INFO_PAIRING only, not of the option */ };
enum { NBODY_COMM_RING = 0,        /* P-1 ncclSend/ncclRecv ring steps, one event per arriving slice */
       NBODY_COMM_ALLGATHER = 1,   /* one in-place ncclAllGather (needs N divisible by the rank count, else ring) */
       NBODY_COMM_AUTO = 2,        /* default: ONE RCCL kernel per step, enqueued ahead of the force launch — ALLGATHER (RCCL's own ring over
                                      xGMI) when N is divisible by the rank count, DIRECT otherwise (profiles/r03_comm_under_load.md:
                                      a transfer kernel enqueued beside a force launch that fills every CU waits for wave slots, and
                                      P-1 dependent ring groups wait P-1 times) */
       NBODY_COMM_DIRECT = 3       /* one group of P-1 sends of the own slice and P-1 receives: one hop over all xGMI links */ };

/* ---- info keys (nbody_get_info) ---- */
enum { NBODY_INFO_N = 1, NBODY_INFO_N_LOCAL, NBODY_INFO_FIRST_BODY, NBODY_INFO_RANK, NBODY_INFO_NRANKS,
       NBODY_INFO_VARIANT, NBODY_INFO_IBLOCK, NBODY_INFO_JSUB, NBODY_INFO_NSEG, NBODY_INFO_DEVICE,
       NBODY_INFO_CU_COUNT, NBODY_INFO_CLOCK_KHZ, NBODY_INFO_FP64, NBODY_INFO_TILE, NBODY_INFO_STEPS_DONE,
       NBODY_INFO_SUM_ORDER, NBODY_INFO_SUM_BLOCK, NBODY_INFO_LAUNCHES_PER_STEP /* kernel launches one nbody_step() step takes */,
       NBODY_INFO_HAS_COMM /* 1: an RCCL communicator exists */,
       NBODY_INFO_WSPLIT /* resolved NBODY_OPT_WSPLIT: 1, 4 or 16 */, NBODY_INFO_ISA_PHASE, NBODY_INFO_LONG_BUFFERS /* option value, -1 = auto */,
       NBODY_INFO_XCD_MAP /* option value, -1 = auto */, NBODY_INFO_FUSE_COMBINE /* resolved: 1 = in-launch combine */,
       NBODY_INFO_COMM_FORM /* resolved NBODY_COMM_* of a multi-rank context, -1 with one rank */,
       NBODY_INFO_COMM_PRIORITY /* HIP priority of the transfer stream (0 = default priority) */,
       NBODY_INFO_DIAG_BUILD /* 1: this is libnbody_hip_diag.so (timing-only loop forms present) */,
       NBODY_INFO_MAILBOX_SERVED /* requests the mailbox's service thread has completed in this process */,
       NBODY_INFO_MAILBOX_SERVING /* 1: nbody_mailbox_serve(1, .) is in effect */,
       NBODY_INFO_MASSES /* NBODY_OPT_MASSES: 0 or 1 */ };
/* (a list of its own: the list above ends with NBODY_INFO_MASSES) */
enum { NBODY_INFO_PAIRING = 31 /* what a step of the context takes: NBODY_PAIRING_ORDERED, NBODY_PAIRING_MUTUAL, or NBODY_PAIRING_NO_TABLE:
                                  MUTUAL was chosen but its table could not be allocated, the pass runs ORDERED */ };

/* ---- lifetime ----
 * Replaces: power-up of the PL design + the ps_pl RAM allocation (S/top_level.vhd:100-117, 148-163). */

/* One process driving `ngpus` devices (ngpus = 1: device NBODY_DEVICE or 0).  tile: LDS tile in
 * bodies for NBODY_VARIANT_LDS (64..1024, multiple of 64; 0 = 256). */
int nbody_init(int n, int ngpus, int fp64, int tile);
/* One process per GPU (the torch.distributed / MPI launch): rank 0 calls nbody_unique_id() and
 * broadcasts the 128 bytes by its own means; every rank then calls nbody_init_rank().  Device =
 * NBODY_DEVICE, else LOCAL_RANK, else rank modulo the visible device count. */
int nbody_unique_id(void *uid128);
int nbody_init_rank(int n, int fp64, int tile, int rank, int nranks, const void *uid128);
/* Transport self-test on the communicator nbody_init_rank created (uid128 != NULL, any nranks >= 1): an in-place
 * all-gather of a patterned array in the configured NBODY_OPT_COMM form and one grouped ncclSend/ncclRecv ring step,
 * every received word checked.  Collective: every rank calls it.  *bytes_moved (may be NULL) = bytes this rank received. */
int nbody_comm_selftest(long long *bytes_moved);
/* The transfer plans of `vranks` VIRTUAL ranks (2..16; a job of that many ranks over this context's N bodies, ragged slices
 * included) in form NBODY_COMM_RING or NBODY_COMM_DIRECT, executed through real ncclSend/ncclRecv on the ONE-rank
 * communicator of nbody_init_rank(..., nranks = 1, uid): each virtual rank has its own array holding its own slice, every
 * receive is issued with the send its peer's plan pairs with it, and afterwards every array must hold all N words.  How a
 * one-GPU box runs the P > 1 offsets, byte counts and pairing of the data path. */
int nbody_comm_selftest_virtual(int vranks, int form, long long *bytes_moved);
/* NBODY_ARITH_STRICT in binary32 evaluates 1/sqrt to the value (float)(1.0 / sqrt((double)x)) — IEEE square root and divide in binary64,
 * rounded once — from eight binary32 operations, and falls back to that expression itself for the ~2^-16 of arguments whose value lies too
 * close to a rounding boundary to be decided that way (csrc/nbody_kernels.hpp rsqrt_strict_f32).  nbody_rsqrt_selftest() proves it on the
 * device: for each of the `count` binary32 BIT PATTERNS first_bits, first_bits + 1, ... (count <= 2^32 covers every float) it evaluates both
 * and counts the patterns where the eight-operation value was accepted and differs (*mismatches: must be 0; *first_bad = the smallest such
 * pattern) and the patterns sent to the IEEE form (*ieee_lanes).  Any pointer may be NULL.  Needs no context (it runs on the context's
 * first device, or on the device a one-GPU context would take).
 * nbody_strict_proof(): THE GATE.  That comparison over every positive normal binary32 (first_bits 0x00800000, count 0x7F000000: 10 ms),
 * on EVERY device of the open context (without a context: on the device a one-GPU context would take), cached per device for the
 * life of the process.  NBODY_OK: proved everywhere; NBODY_ERR_UNSUPPORTED: some device returned a different value (*mismatches,
 * *first_bad — either may be NULL — say how many and where).  The library calls it itself: nbody_set_option(NBODY_OPT_ARITH, a strict
 * mode) in an fp32 context and nbody_mailbox_open(., 1) answer NBODY_ERR_UNSUPPORTED and leave the arithmetic as it was unless every
 * device of the context has proved it — no host layer has to remember the check.
 * nbody_rsqrt_strict(): y[i] = that 1/sqrt of x[i], n values through host pointers, as the force kernels evaluate it (ieee_only = 0) or by
 * the IEEE expression alone (1) — the test surface that ties both to the CPU oracle. */
int nbody_rsqrt_selftest(unsigned first_bits, unsigned long long count, unsigned long long *mismatches, unsigned long long *ieee_lanes, unsigned *first_bad);
int nbody_rsqrt_strict(const float *x, float *y, int n, int ieee_only);
int nbody_strict_proof(unsigned long long *mismatches, unsigned *first_bad);
/* The transfer plan nbody_step() executes for rank `rank` of `nranks` over n bodies (form NBODY_COMM_RING or _DIRECT):
 * 7 values per send/receive pair {group, send_peer, send_first_word, send_words, recv_peer, recv_first_word, recv_words},
 * pairs of one group go into one ncclGroupStart/End.  Pure host arithmetic: needs no GPU and no context.  ops may be NULL
 * (count only); *n_ops = nranks - 1. */
int nbody_comm_plan(int form, int rank, int nranks, int n, long long *ops, int max_ops, int *n_ops);
/* One RCCL ring step (grouped ncclSend to rank+1 / ncclRecv from rank-1) of `bytes` on the transfer stream, timed with HIP
 * events: when = 0 alone, 1 enqueued just before a full force pass, 2 just after it (the force launch occupies every CU)
 * — enqueue to completion; 3 = the steady state of a multi-GPU step (ring step and the next force pass both released by
 * the end of the previous pass), 4 = the same with the hand-shake nbody_step() uses — from the previous pass's end to the
 * ring step's completion.  *force_ms = duration of the (last) force pass (0 for when = 0).  Needs a communicator. */
int nbody_comm_probe(long long bytes, int when, double *comm_ms, double *force_ms);
void nbody_shutdown(void);

int nbody_set_option(int key, int value);
int nbody_get_info(int key, long long *value);
const char *nbody_error_string(int code);

/* ---- state transfer (host <-> device mirrors) ----
 * Replaces: the PS writing bodies to RAM A words 1..N and reading RAM B (S/top_level.vhd:206-208; S/compute_store.vhd:242).
 * Arrays are always the FULL N bodies, on every rank; a rank keeps its own slice of vel. */
int nbody_upload(const BodySystem *host);
int nbody_download(BodySystem *host);
/* This rank's own bodies only: n_local words of pos and of vel (float or double words as the context was created),
 * no collective.  With one GPU it is the whole system. */
int nbody_download_slice(void *pos_words, void *vel_words);
int nbody_upload_d(const BodySystemD *host);
int nbody_download_d(BodySystemD *host);

/* ---- the path ---- */

/* v_i += dt * sum_j (r_j - r_i) * (|r_j - r_i|^2 + 1e-9f)^(-3/2), all j including i; pos is read-only.
 * Host pointers, n must equal the n of nbody_init.  (upload, force kernel + kick, download of vel.)
 * Replaces one full pass of the FSM, S/top_level.vhd:176-272, followed by the host's kick.
 * bodyForce(_d): NBODY_ERR_UNSUPPORTED while NBODY_OPT_MASSES is 1 (unit masses only), before anything is launched, copied or written. */
int bodyForce(float *pos, float *vel, float dt, int n);
/* r_i += v_i * dt.  Host pointers. */
int integrate(float *pos, const float *vel, float dt, int n);
int bodyForce_d(double *pos, double *vel, double dt, int n);
int integrate_d(double *pos, const double *vel, double dt, int n);

/* Device-resident loop: nsteps x { bodyForce; integrate } on the uploaded state, no host round trip
 * per step; asynchronous (nbody_sync or nbody_download waits).  THE TIMED PATH.
 * nbody_step(_d): NBODY_ERR_UNSUPPORTED while NBODY_OPT_MASSES is 1 (unit masses only), before anything is launched, copied or written. */
int nbody_step(float dt, int nsteps);
int nbody_step_d(double dt, int nsteps);
int nbody_sync(void);

/* Force-only entry point with the reference's word layouts: pos_words = N x {x, y, z, ignored}
 * (S/top_level.vhd:206-208), force_words = N x {Fx, Fy, Fz, 0} (S/compute_store.vhd:213, 242).
 * nbody_forces(_d): NBODY_ERR_UNSUPPORTED while NBODY_OPT_MASSES is 1 (unit masses only), before anything is launched, copied or written. */
int nbody_forces(const float *pos_words, float *force_words, int n);
int nbody_forces_d(const double *pos_words, double *force_words, int n);
/* Forces on `n_rows` bodies starting at `first_row`, from the state already on the device (row-sampled parity checks at
 * N = 1M).  first_row: in an nbody_init context (one process, one or several devices) the GLOBAL body index — the range may
 * span devices; in an nbody_init_rank context the row within this rank's own slice.
 * nbody_forces_rows(_d): NBODY_ERR_UNSUPPORTED while NBODY_OPT_MASSES is 1 (unit masses only), before anything is launched, copied or written. */
int nbody_forces_rows(int first_row, int n_rows, float *force_words);
int nbody_forces_rows_d(int first_row, int n_rows, double *force_words);

/* ---- the reference's mailbox (its ONLY interface): the protocol the RTL intends ----
 * RAM A = capacity + 1 words of 16 bytes: word 0 = control {bit 0 BEGIN, bits 46:32 NUM_PTS}, words 1..N = {x, y, z, ignored}
 * (S/top_level.vhd:184-185, 206-208).  RAM B = capacity + 1 words: word k = {Fx, Fy, Fz, 0} of body k — the index the body has in RAM A —
 * and word 0 is NEVER written (S/compute_store.vhd:213, 221-242: write_we and STORE_PTR + 1 are registered on the same edge and write_addr
 * is formed from STORE_PTR combinationally, so the RAM samples we = 1 with the incremented address; the cycle model of those lines is
 * tests/test_fpga_store_model.py.  The signal's name, ZERO_PTR, :76-77, suggests the author meant word k - 1; the RTL does not do it.)
 * "The protocol the RTL intends", not "the RTL verbatim": the sequencer as written breaks that protocol in six places (NUM_PTS <= 3 is
 * never streamed, uninitialised pointers, `waiting` polls word 1, a stale BEGIN starts a second pass, NUM_PTS >= 32761 never ends,
 * `complete` overtakes the last block-group's stores) — shown cycle by cycle in tests/test_fpga_fsm_model.py, listed with what this
 * library does instead in INTEGRATION.md ("Departures from the RTL as written").  None of them is reproduced.
 *
 * nbody_mailbox_open(capacity, faithful): power-up of the PL block — ONE context that then serves any number of requests of any size.
 *   capacity = body words of the two RAMs, 1..32767 (= ram_depth - 1, S/top_level.vhd:45); 0 means 32767.  Replaces any open context.
 *   faithful = 1: the PL block's own bits — NBODY_ARITH_REFERENCE_STRICT (the RTL's rounding points, S/dxy.vhd:113-122, S/dzsoft.vhd:201-202,
 *   S/dxyz_soft.vhd:149-150, 1/sqrt rounded once) + NBODY_SUM_FPGA16 (sixteen partial sums, rotation, adder tree: S/fxyz.vhd:129-184,
 *   S/final_adder.vhd:88-104) + NBODY_OPT_JSUB 1 (one stream of all N sources per body, S/top_level.vhd:233-254) — granted only after the
 *   device has proved the strict 1/sqrt (nbody_strict_proof; NBODY_ERR_UNSUPPORTED and no context otherwise).  faithful = 0: the
 *   engine's timed arithmetic (every force within 1e-5 of the RTL's, not bit-equal).  nbody_shutdown() closes it.
 * nbody_mailbox_rams(): the context's own RAM images — pinned host memory the device reads (RAM A) and writes (RAM B, and word 0 of RAM A
 *   on completion) directly, the PS's view of the two block RAMs (S/top_level.vhd:100-117, 148-163).  A driver that fills *ram_a and passes
 *   these two pointers to nbody_mailbox_run moves no byte on the host; any other host buffers (of NUM_PTS + 1 words each) are accepted too
 *   and cost one host copy each way.  *capacity (may be NULL) = the largest NUM_PTS the context takes.  Works in any one-GPU fp32 context
 *   (nbody_init(n, 1, 0, .): capacity n).
 * nbody_mailbox_run(ram_a, ram_b, clock_khz): ONE request, synchronous (one request in flight, S/top_level.vhd:180-186).
 *   NUM_PTS is sampled from word 0 with every request (S/top_level.vhd:180-186): any value 0..capacity, request after request, on the
 *   same context — 1, 2 and 3 included (the RTL as written stores nothing for those: a stated departure).  Word 0 of RAM B and the words
 *   beyond NUM_PTS are never written (S/compute_store.vhd:221-242); NUM_PTS = 0 completes at once with RAM B untouched
 *   (S/top_level.vhd:189-192).  On return word 0 of ram_a is {ticks in bits 63:32, 0 elsewhere} — BEGIN reads 0.
 *   COMPLETION IS THE DEVICE'S, as in the PL block (S/top_level.vhd:121-146, 255-263): the last launch of a request rewrites word 0 of the
 *   pinned RAM A itself — ticks = 1 + the elapsed 1000-clock units of a `clock_khz` clock (0: 300 MHz) between the first wave that reads
 *   RAM A and that store, counted on the device's real-time counter — and clears BEGIN last, after every word of RAM B; the host only
 *   polls memory.  (NUM_PTS = 0, a refused request, a context over several ranks: the host writes word 0, ticks from its own clock.)
 *   Returns NBODY_ERR_STATE if BEGIN is not set (the FSM stays in `waiting`: nothing read, nothing written), NBODY_ERR_ARG if NUM_PTS
 *   exceeds the capacity (the RTL has no such case: its RAM always holds 32767 bodies).
 *   The context's N, options, uploaded state's size and step graph are as before on return.  Its position buffer is overwritten, as by
 *   nbody_forces, except by a request that reads RAM A in place and leaves the buffer as it was: the faithful mode with the device's
 *   completion and NUM_PTS <= NBODY_MAILBOX_DIRECT_MAX (environment; 256 by default).  A context over several devices or ranks keeps its
 *   fixed N (NUM_PTS must equal it).
 * nbody_mailbox_serve(on, clock_khz): the mailbox WITHOUT a call per request.  on = 1: a library thread takes the place of the PL block's
 *   FSM — it samples word 0 of the context's own RAM A (nbody_mailbox_rams) as the RTL does every clock (S/top_level.vhd:180-186) and runs
 *   each request it finds exactly as nbody_mailbox_run would; the device rewrites word 0 (ticks in bits 63:32, BEGIN cleared LAST, so
 *   whoever reads BEGIN = 0 also reads the ticks and RAM B).  The driver then only writes memory — bodies, then word 0 with NUM_PTS and
 *   BEGIN — and polls word 0, as the PS does.  A request the library cannot take (NUM_PTS beyond the capacity, a device error) completes
 *   with ticks = 0 and the error code in bits 127:96 of word 0, which the RTL always writes as 0.
 *   WHILE SERVING THE THREAD OWNS THE CONTEXT: every entry point that launches, copies or reconfigures (nbody_init*, nbody_mailbox_open,
 *   nbody_mailbox_run, nbody_set_option, nbody_upload*, nbody_download*, nbody_step*, nbody_sync, bodyForce*, integrate*, nbody_forces*,
 *   nbody_kernel_time, nbody_comm_*, nbody_device_ptr, the 1/sqrt self-tests) answers NBODY_ERR_STATE from any other thread;
 *   nbody_get_info reports the context's own N and configuration (never a request's), NBODY_INFO_MAILBOX_SERVED counts completed
 *   requests; nbody_mailbox_rams, nbody_error_string, nbody_mailbox_serve and nbody_shutdown stay available.  on = 0 (and
 *   nbody_shutdown) stops and joins the thread.  The idle thread backs off from spinning to 50-us naps after ~0.1 s without a request.
 *   One-GPU fp32 contexts only.
 * nbody_mailbox_run and nbody_mailbox_serve(1, .): NBODY_ERR_UNSUPPORTED while NBODY_OPT_MASSES is 1 (unit masses only), before anything is launched, copied or written.  A request is the reference's force pass.
 *   nbody_mailbox_open opens a fresh context and thereby resets the option to 0, like every other option. */
int nbody_mailbox_open(int capacity, int faithful);
int nbody_mailbox_rams(void **ram_a, void **ram_b, int *capacity);
int nbody_mailbox_run(void *ram_a, void *ram_b, int clock_khz);
int nbody_mailbox_serve(int on, int clock_khz);

/* Multi-process transport without RCCL: call nbody_init_rank(..., uid128 = NULL), then register a function that
 * all-gathers a host array in place: on entry host_words[first..first+count) of this rank are valid (words of word_bytes
 * bytes, slices as nbody_get_info FIRST_BODY / N_LOCAL), on return all n_total words must be.  Returns 0 on success.
 * Slower (PCIe + the host framework's collective) but needs nothing from the GPU fabric; also what the two-process
 * GPU test uses on a one-GPU box. */
typedef int (*nbody_host_gather_fn)(void *user, void *host_words, int n_total, int word_bytes, int rank, int nranks);
int nbody_set_host_gather(nbody_host_gather_fn fn, void *user);

/* Sum of HIP-event durations of the force kernels since the last reset (NBODY_OPT_TIMING = 1). */
int nbody_kernel_time(double *ms_total, long long *launches, int reset);

/* Exposed communication: how long the compute stream sat waiting for arriving slices since the last reset (HIP events
 * around every such wait, NBODY_OPT_TIMING = 1).  0 when everything arrived while the own-slice kernel was running. */
int nbody_comm_time(double *wait_ms_total, long long *waits, int reset);

/* Device pointers of the resident state (for zero-copy interop with a framework that owns a view):
 * which = 0 current positions (full N), 1 velocities (own slice), 2 last forces (own slice). */
int nbody_device_ptr(int which, void **ptr, size_t *bytes);

/* ---- energy and potential: diagnostics of the state on the device (not in the reference) ----
 * Unit masses, G = 1, eps = the force's softening (the binary32 with bits 0x3089705F, added to d2 exactly as the force adds it), so
 * that the force the library computes is -grad phi of
 *   phi_i = -sum_{j != i} (|r_j - r_i|^2 + eps)^(-1/2)    (the self pair is excluded exactly; coincident distinct bodies give 1/sqrt(eps))
 *   U = 1/2 sum_i phi_i,   T = 1/2 sum_i |v_i|^2,   P = sum_i v_i,   L = sum_i r_i x v_i.
 * Pair arithmetic follows NBODY_OPT_ARITH: d2 in the FMA3 form or the reference's five roundings; 1/sqrt by v_rsq_f32, or under a
 * strict mode the IEEE value (float)(1.0 / sqrt((double)d2)).  fp64 contexts: the fma-contracted d2; the v_rsq_f64 seed refined to
 * full precision by one third-order step, or under a strict mode IEEE sqrt and divide.
 * ORDER (fixed by N alone; the variant, JSUB, JSLICES, WSPLIT, SUM_ORDER and the number of ranks play no part, so phi_i has the same
 * bits however the context is sharded):
 *   level 1: the sources in blocks of 1024 consecutive bodies, each block summed from zero in ascending j in the context precision,
 *            j = i skipped;
 *   level 2: the block sums converted to fp64 and added in ascending block order from zero, giving S_i;  phi_i = 0 - S_i, returned
 *            rounded to the context precision.
 *   Totals are accumulated in fp64 from the fp64 values (U from 0 - S_i, T from fma(vx, vx, fma(vy, vy, vz * vz))): the rows of a rank's
 *   slice in groups of 256 from its first body, each group summed in ascending rows, the groups' sums in ascending order, T and U halved;
 *   then the ranks' eight values added in rank order on every rank, so every rank returns the same bits, equal to those of a one-process
 *   nbody_init(n, P, ., .) context (the totals of different rank counts agree to rounding).  No atomics: two calls return identical bits.
 * nbody_energy(): out[NBODY_ENERGY_WORDS] of the whole system.  nbody_potential_rows(_d)(): phi of n_rows bodies from first_row, rows
 * as in nbody_forces_rows.  Both bring the other slices' positions first (collective in nbody_init_rank contexts: every rank calls
 * them) and leave the step state as it was: positions, velocities, the captured step graph and the force-kernel timer
 * (nbody_kernel_time does not count energy launches).  NBODY_ERR_NOT_INIT without a context, NBODY_ERR_ARG for a null pointer or a bad
 * range, NBODY_ERR_STATE for the other precision's entry point or while the mailbox is served.
 * With NBODY_OPT_MASSES: m_j = the w of body j's position word.  The level-1 sum of a row is s = fma(m_j, inv, s) in ascending j in the
 * context precision — one operation where the unit-mass sum has its add — and for j == i s keeps its value (a select on s, not a
 * zero term: with masses of either sign "adding 0" would not carry the argument); blocks, level 2 and phi_i = 0 - L2_i as above, so
 * nbody_potential_rows returns phi_i = -sum_{j != i} m_j inv, per unit mass.  The totals' per-row terms are formed in binary64 from
 * mi = (double)w_i, one plain binary64 product more each: mi * fma(vx, vx, fma(vy, vy, vz * vz)), mi * phi_i, mi * vx (vy, vz),
 * mi * (y * vz - z * vy) (and its cyclic permutations); groups, ranks and their order are unchanged, so T = 1/2 sum m |v|^2,
 * U = 1/2 sum m_i phi_i, P = sum m v, L = sum m r x v.  NBODY_ENERGY_WORDS stays 8. */
enum { NBODY_ENERGY_KINETIC = 0, NBODY_ENERGY_POTENTIAL, NBODY_ENERGY_PX, NBODY_ENERGY_PY, NBODY_ENERGY_PZ,
       NBODY_ENERGY_LX, NBODY_ENERGY_LY, NBODY_ENERGY_LZ, NBODY_ENERGY_WORDS };
int nbody_energy(double *out);
int nbody_potential_rows(int first_row, int n_rows, float *phi);
int nbody_potential_rows_d(int first_row, int n_rows, double *phi);

/* ---- field at arbitrary points: acceleration and potential of the bodies on the device where the caller asks (not in the reference) ----
 * For a point x and the N bodies on the device, unit masses, G = 1, eps the force's softening (bits 0x3089705F):
 *   a(x)   =  sum_j (r_j - x) * (|r_j - x|^2 + eps)^(-3/2)
 *   phi(x) = -sum_j (|r_j - x|^2 + eps)^(-1/2)
 * over ALL j: a point is not a body, so nothing is excluded by default.  A point that coincides with a body gets +0 from that body in a
 * and 1/sqrt(eps) in -phi.  skip[p] = a global body index leaves that body out of point p's sums (-1: nothing); with points[p] = r_i
 * and skip[p] = i, phi is the phi_i of nbody_potential_rows bit for bit, in every arithmetic.  What it is for: potential or
 * acceleration maps on a line, slice or grid, tracer particles, profiles, the force against the gradient of the potential.
 * Pair arithmetic follows NBODY_OPT_ARITH exactly as the potential's: dx = xj - x (dy, dz likewise), d2 in the FMA3 form or the
 * reference's five roundings, inv = v_rsq_f32(d2) or under a strict mode (float)(1.0 / sqrt((double)d2)), then the force's cube
 * inv2 = inv * inv, inv3 = inv * inv2.  fp64 contexts: the fma-contracted d2; inv the v_rsq_f64 seed refined by the potential's one
 * third-order step, or under a strict mode IEEE sqrt and divide; the same cube.
 * ORDER (fixed by N alone; it is the potential's):
 *   level 1: the sources in blocks of 1024 consecutive bodies; per block four accumulators from +0 in ascending j in the context
 *            precision: ax = fma(dx, inv3, ax), ay and az likewise, s = s + inv; for j == skip[p] all four keep their values;
 *   level 2: the blocks' four sums converted to fp64 and added in ascending block order from zero; accel = (T){A}, phi = (T)(0 - S).
 * The bits of a point's result depend on the N source positions, the point, its skip, the arithmetic and the precision — not on m, on
 * where the point stands in the array, on the launch shape (NBODY_FIELD_SPLIT below), on the force configuration (variant, JSUB,
 * JSLICES, WSPLIT, SUM_ORDER) or on the device or rank count.  No atomics: two calls return identical bits.
 * points: m words {x, y, z, ignored} in the context precision, host memory.  accel: m words {ax, ay, az, 0}, or NULL.  phi: m values, or
 * NULL (at least one of the two).  skip: NULL, or m ints, each -1 or a global body index in [0, N).
 * nbody_init over several devices: the points are divided over the devices in contiguous ranges.  nbody_init_rank: every rank evaluates
 * the points IT was given on its own device; the call is collective only because the other slices' positions are brought first — every
 * rank calls it, m may differ between ranks.  Like the energy entry points it leaves positions, velocities, the arrival counters, the
 * captured step graph and the force-kernel timer as they were.
 * Environment, read on every call: NBODY_FIELD_SPLIT = k >= 1 walks the sources in min(k, blocks) chunks of whole blocks side by side
 * (unset or 0: chosen from m and the CU count, so that few points still fill the device); NBODY_FIELD_SCRATCH_MB (default 256) bounds the
 * per-block sums a split launch stores, larger calls go in consecutive batches of points.  Same bits in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched, for points == NULL, m < 1, both outputs
 * NULL or a skip value outside [-1, N); NBODY_ERR_STATE for the other precision's entry point or while the mailbox is served.
 * With NBODY_OPT_MASSES (m = the w of source j's position word; the w of a `points` word is still ignored): w3 = m * inv3, one more
 * rounding in the context precision, then ax = fma(dx, w3, ax), ay and az likewise, and s = fma(m, inv, s).  Order of the sums, skip,
 * blocks, level 2 and stores are unchanged: accel = sum m_j d inv^3, phi = -sum m_j inv. */
int nbody_field(const float *points, int m, const int *skip, float *accel, float *phi);
int nbody_field_d(const double *points, int m, const int *skip, double *accel, double *phi);

/* ---- tidal tensor at arbitrary points: the gradient of the field, T = grad a = -grad grad phi (not in the reference) ----
 * For a point x and the N bodies on the device, unit masses, G = 1, eps the force's softening (bits 0x3089705F):
 *   d = r_j - x,  inv = (|d|^2 + eps)^(-1/2),  inv2 = inv * inv,  inv3 = inv * inv2,  inv5 = inv3 * inv2
 *   T_ab(x) = d a_a / d x_b = sum_j ( 3 d_a d_b inv5 - delta_ab inv3 )
 * over ALL j, as the field's sums; skip[p] = a global body index leaves that body out of point p's sums (-1: nothing), exactly as in
 * nbody_field.  T is symmetric: the result has six values per point in the order {xx, yy, zz, xy, xz, yz}.  PROPERTY: its trace is
 * -3 eps sum_j inv5 (Poisson's equation for the softened bodies: negative, and zero only as eps -> 0).  A point that coincides with a
 * body without skipping it gets +0 from that body off the diagonal and -eps^(-3/2) on it.  What it is for: tidal stretching and tidal
 * radii, the eigenvalue signature of voids, sheets, filaments and knots, the linearised equations of motion, a time-step or softening
 * criterion from |T|.
 * Pair arithmetic follows NBODY_OPT_ARITH exactly as the field's: dx = xj - x (dy, dz likewise), inv as nbody_field states it (d2 in
 * the FMA3 form or the reference's five roundings; v_rsq_f32 or under a strict mode (float)(1.0 / sqrt((double)d2)); fp64 contexts:
 * the fma-contracted d2, the refined v_rsq_f64 seed or under a strict mode IEEE sqrt and divide).  Then, in the context precision T,
 * every operation rounded once:
 *   inv2 = inv * inv;  inv3 = inv * inv2;  inv5 = inv3 * inv2;  w = (T)3 * inv5;  wx = w * dx;  wy = w * dy;  wz = w * dz
 *   qxx = fma(wx, dx, qxx)  qyy = fma(wy, dy, qyy)  qzz = fma(wz, dz, qzz)
 *   qxy = fma(wx, dy, qxy)  qxz = fma(wx, dz, qxz)  qyz = fma(wy, dz, qyz)   s3 = s3 + inv3
 * ORDER (fixed by N alone; it is the potential's):
 *   level 1: the sources in blocks of 1024 consecutive bodies; per block the seven accumulators above from +0 in ascending j; for
 *            j == skip[p] all seven keep their values;
 *   level 2: the blocks' seven sums converted to fp64 and added in ascending block order from zero; then T_aa = (T)(Q_aa - S3), the
 *            subtraction in fp64 and rounded once, and T_ab = (T)Q_ab.
 * The bits of a point's result depend on the N source positions, the point, its skip, the arithmetic and the precision — not on m, on
 * where the point stands in the array, on the launch shape (NBODY_TIDAL_SPLIT below), on the force configuration or on the device or
 * rank count.  No atomics: two calls return identical bits.  DOMAIN: the field's; a square that overflows gives inv = 0 and the pair
 * contributes +0, in every binary32 arithmetic and in both binary64 ones.
 * points: m words {x, y, z, ignored} in the context precision, host memory.  tensor: m x 6 values.  skip: NULL, or m ints, each -1 or a
 * global body index in [0, N).  The points are divided over the devices as nbody_field divides them; nbody_init_rank: every rank
 * evaluates the points IT was given on its own device, the call is collective only because the other slices' positions are brought
 * first — every rank calls it, m may differ between ranks.  It leaves positions, velocities, the arrival counters, the captured step
 * graph and the force-kernel timer as they were.
 * Environment, read on every call: NBODY_TIDAL_SPLIT = k >= 1 walks the sources in min(k, blocks) chunks of whole blocks side by side
 * (unset or 0: chosen from m and the CU count); NBODY_TIDAL_SCRATCH_MB (default 256) bounds the per-block sums a split launch stores,
 * larger calls go in consecutive batches of points.  Same bits in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched or written, for points == NULL,
 * tensor == NULL, m < 1 or a skip value outside [-1, N); NBODY_ERR_STATE for the other precision's entry point or while the mailbox is
 * served.
 * With NBODY_OPT_MASSES (m = the w of source j's position word): w = ((T)3 * inv5) * m, one more rounding; wx, wy, wz and the six fma
 * as above; s3 = fma(m, inv3, s3).  Everything else is unchanged: T_ab = sum m_j (3 d_a d_b inv^5 - delta_ab inv^3). */
int nbody_tidal(const float *points, int m, const int *skip, float *tensor);
int nbody_tidal_d(const double *points, int m, const int *skip, double *tensor);

/* ---- jerk: the time derivative of the acceleration, at rows and at phase-space points (not in the reference) ----
 * For a point x that moves with velocity u and the N bodies on the device (positions r_j, velocities v_j), unit masses, G = 1, eps the
 * force's softening (bits 0x3089705F), d = r_j - x, w = v_j - u, inv = (|d|^2 + eps)^(-1/2):
 *   a(x)    = sum_j d inv^3                                  the acceleration of nbody_field, bit for bit
 *   j(x, u) = da/dt = sum_j ( w inv^3 - 3 (d . w) d inv^5 )
 * over ALL j; skip[p] = a global body index leaves that body out of point p's sums (-1: nothing), exactly as in nbody_field.  What it is
 * for: the Aarseth time step eta |a| / |j|, the predictor of a Hermite scheme, the error estimate of a leapfrog step.  The library adds
 * no integrator on top of it; nbody_step and nbody_step_adaptive are unchanged.
 * Pair arithmetic, in the context precision T, every operation rounded once:
 *   dx = xj - x (dy, dz likewise)      wx = vxj - ux (wy, wz likewise)
 *   inv as nbody_field states it: it follows NBODY_OPT_ARITH (d2 in the FMA3 form or the reference's five roundings; v_rsq_f32 or under a
 *       strict mode (float)(1.0 / sqrt((double)d2)); fp64 contexts: the fma-contracted d2, the refined v_rsq_f64 seed or under a strict
 *       mode IEEE sqrt and divide)
 *   inv2 = inv * inv      inv3 = inv * inv2
 *   rv = fma(dx, wx, fma(dy, wy, dz * wz))           one form in every arithmetic
 *   c = (T)3 * rv         b = c * inv2
 *   tx = fma(-b, dx, wx)  (ty, tz likewise)
 *   ax = fma(dx, inv3, ax)  (ay, az likewise)        the field's three fma, unchanged
 *   jx = fma(tx, inv3, jx)  (jy, jz likewise)
 * ORDER (fixed by N alone; it is the potential's):
 *   level 1: the sources in blocks of 1024 consecutive bodies; per block the six accumulators above from +0 in ascending j; for
 *            j == skip[p] all six keep their values;
 *   level 2: the blocks' six sums converted to fp64 and added in ascending block order from zero, each rounded once to T.
 * The bits of a query's result depend on the N source positions and velocities, the query (x, u), its skip, the arithmetic and the
 * precision, and on nothing else — not on m, on where the query stands in the array, on which of the two forms brings it, on the launch
 * shape (NBODY_JERK_SPLIT below), on the force configuration or on the device or rank count.  No atomics: two calls return identical bits.
 * DOMAIN: a point on a body that moves with that body's velocity gets +0 from it in both outputs; a point on a body with another
 * velocity gets +0 in the acceleration and w eps^(-3/2) in the jerk.  A separation whose square overflows gives inv = 0 and contributes
 * +0 to both as long as 3 rv does not overflow; beyond that b = inf * 0 and the jerk is NaN.  A NaN position or velocity of a body
 * poisons the jerk of every query that does not skip it.
 * nbody_jerk(_d): points and velocities: m words {x, y, z, ignored} and {ux, uy, uz, ignored} in the context precision, host memory.
 *   accel: m words {ax, ay, az, 0}; jerk: m words {jx, jy, jz, 0}; either may be NULL, not both.  skip: NULL, or m ints, each -1 or a
 *   global body index in [0, N).  The points are divided over the devices as nbody_field divides them; nbody_init_rank: every rank
 *   evaluates the queries IT was given on its own device, m may differ between ranks.
 * nbody_jerk_rows(_d): rows exactly as in nbody_timescale_rows (nbody_init: first_row is a global index, the range may span devices;
 *   nbody_init_rank: a row of the rank's own slice).  Row i's query is (r_i, v_i) with skip = i: bit for bit what nbody_jerk returns for
 *   it.  The queries are read from device memory where they lie; nothing makes a round trip through the host.
 * All four bring the other slices' positions first and then ALL N velocities to every device, as nbody_timescale_rows does (one device
 * reads its own; the devices of an nbody_init context copy each other's slices; an nbody_init_rank job gathers them with the transport
 * it uses for positions): an nbody_init_rank job is collective through these two gathers only, every rank calls.  They leave positions,
 * velocities, the arrival counters, the captured step graph and the force-kernel timer as they were.
 * Environment, read on every call: NBODY_JERK_SPLIT = k >= 1 walks the sources in min(k, blocks) chunks of whole blocks side by side
 * (unset or 0: chosen from m and the CU count); NBODY_JERK_SCRATCH_MB (default 256) bounds the per-block sums a split launch stores,
 * larger calls go in consecutive batches of queries.  Same bits in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched or written, for points == NULL,
 * velocities == NULL, both outputs NULL, m < 1, a bad row range or a skip value outside [-1, N); NBODY_ERR_STATE for the other
 * precision's entry point or while the mailbox is served.
 * With NBODY_OPT_MASSES (m = the w of source j's position word; queries and rows-as-queries have no mass): w3 = m * inv3, one more
 * rounding; the field's three fma with w3 and jx = fma(tx, w3, jx), jy and jz likewise; rv, b and t as above.  The acceleration is
 * still nbody_field's bit for bit.  Both are per unit mass of the query, which is what an integrator needs. */
int nbody_jerk(const float *points, const float *velocities, int m, const int *skip, float *accel, float *jerk);
int nbody_jerk_d(const double *points, const double *velocities, int m, const int *skip, double *accel, double *jerk);
int nbody_jerk_rows(int first_row, int n_rows, float *accel, float *jerk);
int nbody_jerk_rows_d(int first_row, int n_rows, double *accel, double *jerk);

/* ---- snap: the second time derivative of the acceleration, at rows and at phase-space points (not in the reference) ----
 * For a point x that moves with velocity u and acceleration a_x and the N bodies on the device (positions r_j, velocities v_j,
 * accelerations a_j), unit masses, G = 1, eps the force's softening, d = r_j - x, w = v_j - u, g = a_j - a_x, inv = (|d|^2 + eps)^(-1/2),
 * alpha = (d . w) inv^2, beta = (w . w + d . g) inv^2 + alpha^2 (Nitadori & Makino 2008):
 *   a(x)          = sum_j A_j,  A_j = d inv^3                          the acceleration of nbody_jerk, bit for bit
 *   j(x, u)       = sum_j J_j,  J_j = w inv^3 - 3 alpha A_j            the jerk of nbody_jerk, bit for bit
 *   s(x, u, a_x)  = d2a/dt2 = sum_j ( g inv^3 - 6 alpha J_j - 3 beta A_j )
 * over ALL j; skip as in nbody_jerk.  The bodies' accelerations a_j are not part of the state: every call first runs the jerk rows pass
 * over all N rows (a_j = the acceleration nbody_jerk_rows returns for row j) and brings the N words to every device; the query's own
 * acceleration a_x is the caller's (points) or a_i (rows).  What it is for: the sixth-order Hermite scheme below and higher-order time
 * step criteria.
 * Pair arithmetic, in the context precision T, every operation rounded once.  d, w, inv, inv2, inv3, rv, c, b, t, the field's three fma
 * and the jerk's three fma are nbody_jerk's to the letter, in every arithmetic; then
 *   gx = axj - ax_x  (gy, gz likewise)
 *   alpha = rv * inv2
 *   q = fma(dx, gx, fma(dy, gy, fma(dz, gz, fma(wx, wx, fma(wy, wy, wz * wz)))))
 *   beta = fma(alpha, alpha, q * inv2)
 *   k6 = (T)6 * alpha     k3 = (T)3 * beta
 *   ux = fma(-k3, dx, fma(-k6, tx, gx))  (uy, uz likewise)
 *   sx = fma(ux, inv3, sx)  (sy, sz likewise)
 * ORDER (fixed by N alone; it is the potential's):
 *   level 1: the sources in blocks of 1024 consecutive bodies; per block the nine accumulators from +0 in ascending j; for
 *            j == skip[p] all nine keep their values;
 *   level 2: the blocks' nine sums converted to fp64 and added in ascending block order from zero, each rounded once to T.
 * The bits of a query's result depend on the N source positions and velocities, the query (x, u, a_x), its skip, the arithmetic and the
 * precision, and on nothing else — not on m, on where the query stands in the array, on which of the two forms brings it, on the launch
 * shape (NBODY_SNAP_SPLIT, NBODY_JERK_SPLIT), on the force configuration or on the device or rank count.  No atomics.
 * DOMAIN: a point on a body that moves with that body's velocity and acceleration gets +0 from it in all three outputs; with another
 * acceleration it gets g eps^(-3/2) in the snap.  A separation whose square overflows gives inv = 0 and contributes +0 to all three as
 * long as no product with it overflows; beyond that inf * 0 makes the jerk or the snap NaN.  A NaN position, velocity or acceleration of
 * a body poisons the snap of every query that does not skip it — and a NaN position or velocity of ANY body, skipped or not, reaches
 * the snap of every query through the accelerations a_j of the bodies beside it.
 * nbody_snap(_d): points, velocities, accelerations: m words {., ., ., ignored} each in the context precision, host memory.  accel, jerk,
 *   snap: m words {., ., ., 0} each; any may be NULL, not all three.  skip and the division of the points over devices and ranks as in
 *   nbody_jerk.
 * nbody_snap_rows(_d): rows exactly as in nbody_jerk_rows.  Row i's query is (r_i, v_i, a_i) with skip = i: bit for bit what nbody_snap
 *   returns for it.  Nothing makes a round trip through the host.
 * All four bring positions and velocities as nbody_jerk does, run the jerk rows pass on every device's own rows, bring ALL N
 * accelerations to every device the same way (one device reads its own; the devices of an nbody_init context copy each other's; an
 * nbody_init_rank job gathers them with the transport it uses for positions and then gathers the velocities again) and run the snap
 * pass: two all-pairs passes per call.  An nbody_init_rank job is collective through the gathers only, every rank calls.  They leave
 * positions, velocities, the arrival counters, the captured step graph and the force-kernel timer as they were.
 * Environment, read on every call: NBODY_SNAP_SPLIT and NBODY_SNAP_SCRATCH_MB as NBODY_JERK_SPLIT and NBODY_JERK_SCRATCH_MB, for the
 * snap pass (nine sums per point and block); the opening jerk pass follows its own two.  Same bits in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched or written, for points == NULL,
 * velocities == NULL, accelerations == NULL, all three outputs NULL, m < 1, a bad row range or a skip value outside [-1, N);
 * NBODY_ERR_STATE for the other precision's entry point or while the mailbox is served.
 * With NBODY_OPT_MASSES (m = the w of source j's position word): w3 = m * inv3 as in nbody_jerk, and sx = fma(ux, w3, sx); the opening
 * jerk pass is weighted too, so the a_j are the weighted accelerations.  All three outputs are per unit mass of the query. */
int nbody_snap(const float *points, const float *velocities, const float *accelerations, int m, const int *skip, float *accel, float *jerk, float *snap);
int nbody_snap_d(const double *points, const double *velocities, const double *accelerations, int m, const int *skip, double *accel, double *jerk, double *snap);
int nbody_snap_rows(int first_row, int n_rows, float *accel, float *jerk, float *snap);
int nbody_snap_rows_d(int first_row, int n_rows, double *accel, double *jerk, double *snap);

/* ---- fourth-order Hermite integrator: predict, evaluate, correct on the jerk pass (not in the reference) ----
 * nbody_step is a kick followed by a drift: first order.  nbody_step_hermite(_d) advances the state on the device by nsteps steps of
 * the Makino–Aarseth Hermite scheme in its PEC form with a shared dt: one jerk rows pass per step plus one at the start of the call.
 * T is the context precision; every operation is rounded once, products are fused only where fma is written.
 *   start of a call   (a0, j0) of every row at (r, v): exactly what nbody_jerk_rows returns (skip = self, arithmetic after NBODY_OPT_ARITH)
 *   coefficients      once per step in T from h = dt:  h2 = h * h   c2 = h2 * (T)0.5   c3 = (h2 * h) / (T)6   hh = h * (T)0.5
 *                     c12 = h2 / (T)12   (IEEE quotients)
 *   predict           xp = fma(c3, j0, fma(c2, a0, fma(h, v0, x0)))      vp = fma(c2, j0, fma(h, a0, v0))        per component
 *   evaluate          (a1, j1): the same rows pass over the predicted state — the predicted positions and velocities of all N bodies are
 *                     the sources, row i's query is (xp_i, vp_i) and leaves itself out
 *   correct           v1 = fma(c12, j0 - j1, fma(hh, a0 + a1, v0))      x1 = fma(c12, a0 - a1, fma(hh, v0 + v1, x0))   per component
 *   carried           the position word's w bit for bit; the velocity word's fourth value stays as it is
 *   next step         (a0, j0) := (a1, j1): the usual PEC form does not evaluate again at the corrected state
 * A CALL IS STATELESS: it evaluates (a0, j0) afresh from the state it finds, so nothing has to be invalidated by uploads, nbody_step or
 * the mailbox.  A call of k steps takes k + 1 passes; k calls of one step are k restarts, take 2k passes and in general give other bits
 * than one call of k steps.  Both are defined by the statement above.
 * The jerk pass's sums are ordered by N alone and the predictor and corrector are elementwise, so a Hermite step — unlike nbody_step, whose
 * sums follow the launch configuration — gives the same bits on one device, on several, in an nbody_init_rank job of any size and under
 * any source split (NBODY_JERK_SPLIT, NBODY_JERK_SCRATCH_MB) or force configuration.
 * The call returns with the state written (it is synchronous); NBODY_INFO_STEPS_DONE counts Hermite steps as well.  Afterwards
 * nbody_download, nbody_forces_rows, nbody_jerk_rows and nbody_energy see the corrected state of all bodies, and a later nbody_step
 * gives what it gives on a fresh context uploaded with that state.  Arrival counters, the captured step graph and the force-kernel timer
 * stay as they were.  In an nbody_init_rank job the call is collective (every rank calls with the same arguments) through the position
 * and velocity gathers and the exchange of the ranks' best values only.
 * A negative dt is legal (the scheme runs backwards).  NBODY_ERR_ARG for nsteps < 1 or a dt that is not finite; NBODY_ERR_NOT_INIT without
 * a context; NBODY_ERR_STATE for the other precision's entry point or while the mailbox is served.
 * nbody_min_aarseth (both precisions): runs the rows pass on the current state and, in binary64 from the T values, contraction off,
 * takes per row a2 = (ax*ax + ay*ay) + az*az, j2 likewise and q_i = a2 / j2.  *q = the smallest q_i, *row = the lowest global row that
 * reaches it; a NaN or +inf q_i (j2 = 0) is never chosen; with no candidate *q = +inf and *row = -1.  Either pointer may be NULL, not
 * both (NBODY_ERR_ARG).  The reduction runs on the device in a fixed order; the devices' or ranks' bests are exchanged as
 * nbody_min_timescale exchanges its own and folded in rank order with strict <.  A minimum is exact: the same values on every rank, for
 * every device count and split.
 * nbody_step_hermite_adaptive(_d): the shared Aarseth step, in the shape of nbody_step_adaptive: from t = 0, everything but the step in
 * binary64 on the host.  After the opening evaluation and after every step, while t < t_end and fewer than max_steps steps were taken:
 *     q = the minimum above over the (a, j) the integrator carries (no extra pass);  h = eta * sqrt(q);  h = min(h, dt_max);
 *     h = max(h, dt_min);  if (t + h > t_end) h = t_end - t;  dt = h rounded once to T;  one Hermite step of dt;  t += (double)dt.
 * Argument checks, *t_reached and *steps_taken (either may be NULL) as in nbody_step_adaptive: NBODY_ERR_ARG unless eta, t_end, dt_min
 * and dt_max are finite, eta > 0, 0 < dt_min <= dt_max, t_end > 0 and max_steps >= 1; running into max_steps is no error.
 * With NBODY_OPT_MASSES: nbody_jerk_rows, nbody_step_hermite(_d), nbody_min_aarseth, nbody_step_hermite_adaptive(_d) and
 * nbody_step_hermite_block(_d) inherit the masses from the jerk pass with no code of their own.  The acceleration and the jerk are per
 * unit mass of the row, so predictor, corrector, the Aarseth ratio, the level rule and the counters are unchanged; predictor and
 * corrector carry the w of a position word bit for bit, so the predicted state — the source array of the evaluation — holds the masses,
 * and every gather moves whole words.  A body with w = +0 is a massless tracer: it is accelerated and moves no one. */
int nbody_step_hermite(float dt, int nsteps);
int nbody_step_hermite_d(double dt, int nsteps);
int nbody_min_aarseth(double *q, int *row);
int nbody_step_hermite_adaptive(float eta, float t_end, float dt_min, float dt_max, int max_steps, double *t_reached, int *steps_taken);
int nbody_step_hermite_adaptive_d(double eta, double t_end, double dt_min, double dt_max, int max_steps, double *t_reached, int *steps_taken);

/* ---- sixth-order Hermite integrator: predict, evaluate, correct on the snap pass (not in the reference) ----
 * nbody_step_hermite6(_d) advances the state on the device by nsteps steps of the sixth-order Hermite scheme of Nitadori & Makino (2008)
 * in its PEC form with a shared dt: one snap rows pass per step plus the two passes of nbody_snap_rows at the start of the call.  It
 * carries acceleration a, jerk j, snap s and, for the predictor alone, the crackle c (the third derivative of a).  At the same number of
 * steps it is far more accurate than the fourth-order scheme (Kepler pair, e = 0.5, to t = 1 in 128 steps, binary64: relative energy
 * error 2.7e-10 against 1.8e-7) at about twice the pair arithmetic.  T is the context precision; every operation is rounded once,
 * products are fused only where fma is written.
 *   start of a call   (a0, j0, s0) of every row at (r, v): exactly what nbody_snap_rows returns; c0 = +0
 *   coefficients      once per step in T from h = dt:  h2 = h * h   c2 = h2 * (T)0.5   c3 = (h2 * h) / (T)6   c4 = (h2 * h2) / (T)24
 *                     c5 = ((h2 * h2) * h) / (T)120   hh = h * (T)0.5   c10 = h2 / (T)10   c120 = (h2 * h) / (T)120   r = (T)1 / h
 *                     (IEEE quotients)
 *   predict           xp = fma(c5, c0, fma(c4, s0, fma(c3, j0, fma(c2, a0, fma(h, v0, x0)))))
 *                     vp = fma(c4, c0, fma(c3, s0, fma(c2, j0, fma(h, a0, v0))))
 *                     ap = fma(c3, c0, fma(c2, s0, fma(h, j0, a0)))                                                per component
 *   evaluate          (a1, j1, s1): the snap rows pass over the predicted state — the predicted positions, velocities and accelerations
 *                     of all N bodies are the sources, row i's query is (xp_i, vp_i, ap_i) and leaves itself out
 *   correct           v1 = fma(c120, s0 + s1, fma(c10, j0 - j1, fma(hh, a0 + a1, v0)))
 *                     x1 = fma(c120, j0 + j1, fma(c10, a0 - a1, fma(hh, v0 + v1, x0)))                            per component
 *   crackle           e1 = (T)60 * (a1 - a0)   e2 = fma((T)36, j1, (T)24 * j0)   e3 = fma((T)9, s1, (T)-3 * s0)
 *                     c1 = r * fma(r, fma(r, e1, -e2), e3): the third derivative, at the end of the step, of the quintic through both
 *                     evaluations.  Without it the scheme falls to fifth order
 *   carried           the position word's w bit for bit; the velocity word's fourth value stays as it is
 *   next step         (a0, j0, s0, c0) := (a1, j1, s1, c1)
 * A CALL IS STATELESS, as nbody_step_hermite is: it evaluates (a0, j0, s0) afresh and starts from c0 = +0.  A call of k steps takes k + 2
 * passes; k calls of one step are k restarts, take 3k passes and give other bits than one call of k steps.  Both are defined by the
 * statement above.  Same bits on one device, on several, in an nbody_init_rank job of any size and under any source split
 * (NBODY_SNAP_SPLIT, NBODY_SNAP_SCRATCH_MB, the jerk pass's two) or force configuration.
 * Argument checks, the synchronous return, NBODY_INFO_STEPS_DONE, a negative dt, what later calls see and what stays untouched are as
 * stated for nbody_step_hermite; an nbody_init_rank job is collective through the position, velocity and acceleration gathers and the
 * exchange of the ranks' best values.  dt = 0 divides by zero in r: the state becomes NaN.
 * nbody_step_hermite6_adaptive(_d): nbody_step_hermite_adaptive's loop, arguments, checks and outputs over sixth-order steps, with the same
 * q = min_i |a_i|^2 / |j_i|^2 over the (a, j) the integrator carries.
 * With NBODY_OPT_MASSES everything is inherited from the snap pass, as the fourth-order scheme inherits it from the jerk pass. */
int nbody_step_hermite6(float dt, int nsteps);
int nbody_step_hermite6_d(double dt, int nsteps);
int nbody_step_hermite6_adaptive(float eta, float t_end, float dt_min, float dt_max, int max_steps, double *t_reached, int *steps_taken);
int nbody_step_hermite6_adaptive_d(double eta, double t_end, double dt_min, double dt_max, int max_steps, double *t_reached, int *steps_taken);

/* ---- individual block time steps: the Hermite integrator with a step per body, quantised to powers of two (not in the reference) ----
 * nbody_step_hermite_adaptive gives all N bodies the step of the worst pair.  nbody_step_hermite_block(_d) advances the state on the
 * device by nblocks * dt_max with a step per body: level k has the step dt_max * 2^-k, k = 0 .. levels - 1, and only the bodies that are
 * due are evaluated, against the predicted state of all the others (NBODY6, phiGRAPE, Sapporo).  T is the context precision.
 *   time          integer ticks (64-bit) of unit = dt_max * 2^-(levels - 1), computed in T (exact: it is checked normal).  Row i carries a
 *                 tick t0_i, a level k_i and its base (x0, v0, a0, j0) at t0_i; its step is s_i = 2^(levels - 1 - k_i) ticks.
 *   wanted level  of a row from its (a, j), in binary64, contraction off: q = a2 / j2 as nbody_min_aarseth forms it, e = eta2 * q with
 *                 eta2 = eta * eta from the T value of eta, lim[k] = (d * 2^-k)^2 with d = (double)dt_max; want = the smallest k with
 *                 lim[k] <= e, levels - 1 if there is none, and 0 when q is not < +inf (NaN or +inf: a lone body, a row with zero jerk).
 *                 No square root; the only division is q's.
 *   start         base := the state; (a0, j0) := what nbody_jerk_rows returns; t0 := 0; k := want.
 *   a sub-step    tau := the smallest t0_i + s_i over all rows of all ranks.  Every row is predicted from its base to tau by the
 *                 predictor above with h_i = (T)(tau - t0_i) * unit (the integer is below 2^23 + 1: one rounding) and the coefficients
 *                 of h_i.  The ACTIVE rows, those with t0_i + s_i = tau, are evaluated by the jerk at points: the query is the row's
 *                 predicted (x, v) with skip = its own index, the sources the predicted state of all N bodies.  They alone are
 *                 corrected by the corrector above with their own h_i (= s_i * unit): base := (x1, v1, a1, j1), t0 := tau; then with
 *                 w = want(a1, j1): w > k: k := w;  w < k and tau mod 2^(levels - k) == 0: k := k - 1 (one doubling, onto an aligned
 *                 time only);  otherwise k stays.
 *   end           when tau = nblocks * 2^(levels - 1).  Every t0_i is a multiple of s_i, so no row steps over a multiple of
 *                 2^(levels - 1) and at each such multiple every row is active: the call ends with every body at the same time.
 * With levels = 1 the call is nbody_step_hermite(dt_max, nblocks) bit for bit, in every arithmetic.  Like it the call is stateless
 * ((a0, j0) afresh, levels assigned anew), synchronous, gives the same bits however the work is laid out, leaves alone what
 * nbody_step_hermite leaves alone and is collective in an nbody_init_rank job (a rank without an active row takes part in the gathers).
 * *substeps = the number of distinct times visited, *row_evals = the sum of the active counts over them (the pass at the start of the
 * call is in neither); either may be NULL.  NBODY_INFO_STEPS_DONE advances by the number of sub-steps.
 * NBODY_ERR_ARG, the state untouched: eta or dt_max not finite or <= 0, levels < 1 or > 24, nblocks < 1, dt_max * 2^-(levels - 1) below
 * the smallest normal of T.  NBODY_ERR_NOT_INIT without a context; NBODY_ERR_STATE for the other precision's entry point or while the
 * mailbox is served. */
int nbody_step_hermite_block(float eta, float dt_max, int levels, int nblocks, long long *substeps, long long *row_evals);
int nbody_step_hermite_block_d(double eta, double dt_max, int levels, int nblocks, long long *substeps, long long *row_evals);

/* ---- sixth-order individual block time steps: the sixth-order Hermite integrator with a step per body (not in the reference) ----
 * nbody_step_hermite6_block(_d) joins the two sections above: the sixth-order scheme of nbody_step_hermite6 on the scheduler of
 * nbody_step_hermite_block.  Arguments, checks, return codes and counters are nbody_step_hermite_block's to the letter; the call advances
 * the state on the device by nblocks * dt_max.  T is the context precision; every operation is rounded once, products are fused only
 * where fma is written.
 *   time          as above: integer ticks (64-bit) of unit = dt_max * 2^-(levels - 1), computed in T.  Row i carries a tick t0_i, a level
 *                 k_i and its base (x0, v0, a0, j0, s0, c0) at t0_i, c the crackle; its step is s_i = 2^(levels - 1 - k_i) ticks.
 *   wanted level  as above, from the row's (a, j) alone: the fourth-order ratio q = |a|^2 / |j|^2 — what nbody_step_hermite6_adaptive
 *                 keeps for its shared step too.  The generalised Aarseth criterion of Nitadori & Makino over higher derivatives is not
 *                 implemented.
 *   start         base := the state; (a0, j0, s0) := what nbody_snap_rows returns (its two passes); c0 := +0; t0 := 0; k := want.
 *   a sub-step    tau := the smallest t0_i + s_i over all rows of all ranks.  Every row is predicted from its base to tau with
 *                 h_i = (T)(tau - t0_i) * unit and the sixth-order coefficients of h_i, formed per row exactly as stated above for h
 *                 (IEEE quotients): xp, vp and ap by the three fma chains of the sixth-order predictor.  The ACTIVE rows, those with
 *                 t0_i + s_i = tau, are evaluated by the snap at points: the query is the row's predicted (xp, vp, ap) with skip = its
 *                 own index, the sources the predicted positions, velocities and accelerations of all N bodies.  They alone are
 *                 corrected with their own h_i: v1, x1 and the crackle c1 of the sixth-order corrector with r = (T)1 / h_i;
 *                 base := (x1, v1, a1, j1, s1, c1), t0 := tau; then the level moves as above with w = want(a1, j1).
 *   carried       the position word's w and the velocity word's fourth value bit for bit.
 *   end           as above: when tau = nblocks * 2^(levels - 1), with every body at that time.
 * With levels = 1 the call is nbody_step_hermite6(dt_max, nblocks) bit for bit, in every arithmetic.  Like it the call is stateless
 * ((a0, j0, s0) afresh, c0 = +0, levels assigned anew: two calls of one block give other bits than one call of two), synchronous, gives the
 * same bits however the work is laid out (devices, ranks, NBODY_SNAP_SPLIT, NBODY_SNAP_SCRATCH_MB), never changes the live buffer,
 * launches no force kernel, leaves alone what nbody_step_hermite leaves alone and is collective in an nbody_init_rank job through the
 * position, velocity and acceleration gathers and the exchange of the ranks' next times (a rank without an active row takes part).
 * *substeps, *row_evals (either may be NULL) and NBODY_INFO_STEPS_DONE (one per sub-step) as above; the two passes at the start of the call
 * are in neither counter.  NBODY_ERR_ARG, NBODY_ERR_NOT_INIT and NBODY_ERR_STATE exactly as above, the state untouched.
 * With NBODY_OPT_MASSES everything is inherited from the snap pass; a body with w = +0 is a massless tracer. */
int nbody_step_hermite6_block(float eta, float dt_max, int levels, int nblocks, long long *substeps, long long *row_evals);
int nbody_step_hermite6_block_d(double eta, double dt_max, int levels, int nblocks, long long *substeps, long long *row_evals);

/* ---- nearest neighbour, radius count, closest pair: how close the bodies on the device get (not in the reference) ----
 * A query is a point x with an optional excluded body.  In the context precision T, for every body j on the device:
 *   dx = xj - x;  dy = yj - y;  dz = zj - z;   d2_j = fma(dx, dx, fma(dy, dy, dz * dz))
 * the plain squared distance: no softening is added (a diagnostic of the distance itself: min d2, a time step from d / |v|, a collision
 * candidate must see 0 where two bodies coincide), and it does not follow NBODY_OPT_ARITH — every operation is IEEE-exact, one
 * definition per precision.  Over the N bodies, the body `skip` left out:
 *   idx    the j with the smallest d2_j, on equal values the lowest j: what an ascending scan from (d2 = +inf, idx = -1) that replaces
 *          on strict < arrives at.  A NaN d2_j is never chosen (nor is a d2_j that overflowed to +inf: it is not below +inf).  Without
 *          a candidate (N = 1 with that body skipped, every d2_j NaN): idx = -1, d2 = +inf.
 *   d2     that body's d2_j, in T.  A coincident distinct body gives +0, a legitimate answer.
 *   count  the number of non-skipped j with d2_j <= r2; r2 is given already squared, in T.  NaN is never counted.  r2 = +inf is legal
 *          and counts every j whose d2_j is not NaN, one that overflowed to +inf included (+inf <= +inf) — the same j that is never
 *          chosen as idx and that no edge of the radial counts below holds, a +inf edge included (+inf < +inf is false).
 * A minimum and an integer count are exact: the bits depend on the N positions, the query and its skip alone — not on the number of
 * queries, on where the query stands, on the launch shape (NBODY_NEIGHBORS_SPLIT below), on the arithmetic, on the force configuration
 * or on the device or rank count.  No atomics: two calls return identical values.
 * nbody_neighbors_rows(_d): the queries are the bodies themselves, each excluding itself; rows exactly as in nbody_forces_rows
 *   (nbody_init: first_row is a global index, the range may span devices; nbody_init_rank: a row of the rank's own slice).  The idx
 *   returned are always GLOBAL body indices.  idx, d2 or count may be NULL (at least one is not); count == NULL: no counting, r2 ignored.
 * nbody_nearest(_d): the queries are m caller points; points (m words {x, y, z, ignored}) and skip (NULL, or m ints, -1 or a global
 *   body index) mean what they mean for nbody_field.  A point on a body without a skip finds that body at d2 = +0.  The points are
 *   divided over the devices as the field pass divides them; nbody_init_rank: every rank asks for its own points, m may differ.
 * nbody_closest_pair(_d): the pair i < j with the smallest d2 over the whole system, ties to the lowest i, then the lowest j; N = 1 (or
 *   no comparable pair): i = j = -1, d2 = +inf.  Any of the three may be NULL (not all).  It runs the rows pass over every device's or
 *   rank's own rows and keeps each one's best row by a fixed-order reduction; the winner is picked in rank order with strict <.  In an
 *   nbody_init_rank job it is collective and every rank returns the same values.
 * All three bring the other slices' positions first (collective in nbody_init_rank contexts) and, like the energy and field entry
 * points, leave positions, velocities, the arrival counters, the captured step graph and the force-kernel timer as they were.
 * Environment, read on every call: NBODY_NEIGHBORS_SPLIT = k >= 1 walks the sources in min(k, blocks of 1024) chunks side by side
 * (unset or 0: chosen from the number of queries and the CU count, so that few queries still fill the device);
 * NBODY_NEIGHBORS_SCRATCH_MB (default 256, fractions allowed) bounds the 12 (fp64: 16) bytes per query and chunk a split launch stores,
 * larger calls go in consecutive batches of queries; NBODY_NEIGHBORS_LOOP = 1 | 2 picks the hot loop's form.  Same
 * values in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched, for every output NULL, a bad row range,
 * points == NULL, m < 1 or a skip value outside [-1, N); NBODY_ERR_STATE for the other precision's entry point or while the mailbox
 * is served. */
int nbody_neighbors_rows(int first_row, int n_rows, int *idx, float *d2, float r2, int *count);
int nbody_neighbors_rows_d(int first_row, int n_rows, int *idx, double *d2, double r2, int *count);
int nbody_nearest(const float *points, int m, const int *skip, int *idx, float *d2, float r2, int *count);
int nbody_nearest_d(const double *points, int m, const int *skip, int *idx, double *d2, double r2, int *count);
int nbody_closest_pair(int *i, int *j, float *d2);
int nbody_closest_pair_d(int *i, int *j, double *d2);

/* ---- k nearest neighbours: which k bodies are nearest, and how far away the k-th is (not in the reference) ----
 * The dual of the section above: a local density k / r_k^3, softening or time steps from the k-th neighbour's distance, interpolation
 * stencils, linking lengths.  Queries, skip and d2 are exactly the neighbour pass's: in the context precision T, for every body j,
 *   dx = xj - x;  dy = yj - y;  dz = zj - z;   d2_j = fma(dx, dx, fma(dy, dy, dz * dz))
 * no softening, independent of NBODY_OPT_ARITH, every operation IEEE-exact.
 * A CANDIDATE is a non-skipped j with d2_j < +inf: a NaN d2_j is never listed, nor is one that overflowed to +inf.  For a query and
 * 1 <= k <= NBODY_KNN_MAX the result is the first k candidates in ascending (d2_j, j) order, a total order — what an ascending scan
 * over j arrives at that starts from k entries (d2 = +inf, idx = -1), puts a candidate behind every entry with d2 <= its own and drops
 * the last entry.  Entry 0 is the nearest.  With fewer than k candidates the remaining entries are idx = -1, d2 = +inf.  A coincident
 * distinct body is listed at +0.
 * Entry r of any k equals entry r of any larger k, and entry 0 equals nbody_neighbors_rows / nbody_nearest.  A selection is exact: the
 * values depend on the N positions, the query, its skip and k alone — not on the number of queries, on where the query stands, on the
 * launch shape (NBODY_KNN_SPLIT below), on the arithmetic, on the force configuration or on the device or rank count.  No atomics: two
 * calls return identical values.
 * idx, d2: m (n_rows) x k values, row-major: entry r of query p at [p * k + r]; either may be NULL, not both.
 * nbody_knn_rows(_d): the queries are the bodies themselves, each excluding itself; rows exactly as in nbody_forces_rows and
 *   nbody_neighbors_rows.  The idx returned are always GLOBAL body indices.
 * nbody_knn(_d): the queries are m caller points; points, skip and the division over the devices as in nbody_nearest.  nbody_init_rank:
 *   every rank asks for its own points, m and k may differ between ranks.
 * Both bring the other slices' positions first (collective in nbody_init_rank contexts) and, like their siblings, leave positions,
 * velocities, the arrival counters, the captured step graph and the force-kernel timer as they were.
 * Environment, read on every call: NBODY_KNN_SPLIT = c >= 1 walks the sources in min(c, blocks of 1024) chunks side by side (unset or 0:
 * chosen from the number of queries and the CU count); NBODY_KNN_SCRATCH_MB (default 256, fractions allowed) bounds the k * 8 (fp64:
 * k * 12) bytes per query and chunk a split launch stores, larger calls go in consecutive batches of queries.  Same values in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched or written, for both outputs NULL, k < 1,
 * k > NBODY_KNN_MAX, a bad row range, points == NULL, m < 1 or a skip value outside [-1, N); NBODY_ERR_STATE for the other precision's
 * entry point or while the mailbox is served. */
#define NBODY_KNN_MAX 32
int nbody_knn_rows(int first_row, int n_rows, int k, int *idx, float *d2);
int nbody_knn_rows_d(int first_row, int n_rows, int k, int *idx, double *d2);
int nbody_knn(const float *points, int m, const int *skip, int k, int *idx, float *d2);
int nbody_knn_d(const double *points, int m, const int *skip, int k, int *idx, double *d2);

/* ---- friends-of-friends groups: which bodies belong together at a linking length (not in the reference) ----
 * The sections above answer a question about one body or one point; this one is about the system: halos, clumps, bound-pair candidates,
 * "is the system still one piece".  The pair predicate is the neighbour pass's d2 in the context precision T,
 *   dx = xj - xi;  dy = yj - yi;  dz = zj - zi;   d2_ij = fma(dx, dx, fma(dy, dy, dz * dz))
 * no softening, independent of NBODY_OPT_ARITH, every operation IEEE-exact; it is symmetric bit for bit.
 * Bodies i != j are LINKED when d2_ij <= b2; b2 is the linking length already squared, in T, as r2 is for the radius count.  A NaN d2
 * links nothing, so a NaN body is a group of one; coincident bodies (d2 = +0) are linked for every b2 >= 0.  A GROUP is a connected
 * component of the link graph.
 *   group[i]   the lowest global body index in i's group; group[i] == i for exactly one body per group.  N ints, or NULL.
 *   n_groups   the number of such bodies.  May be NULL (group and n_groups not both).
 *   rounds     the number of link passes the call ran, a diagnostic: the same for two identical calls and for every launch shape.
 *              May be NULL.
 * The result is a property of the N positions and b2 alone: it does not depend on the launch shape (NBODY_FOF_SPLIT below), on the
 * rounds taken, on the force configuration or on the device or rank count.  No atomics: two calls return identical values.
 * How: the all-pairs work runs on the device, the O(N) bookkeeping on the host.  The host keeps a union-find whose root is the lowest
 * index, L[i] = find(i).  A round uploads L, the link pass gives every active row i the lowest FOREIGN label among its friends,
 *   m_i = min{ L[j] : d2_ij <= b2 and L[j] != L[i] }   (INT_MAX: none; the self pair drops out by its label),
 * and the host unites i with m_i.  A round in which no row reports is the last.  Every group that is not yet a whole component has a
 * row that reports, so the incomplete groups at least halve per round: rounds <= ceil(log2 N) + 1, a hard cap of the host loop
 * (NBODY_ERR_STATE beyond it; nothing on the device spins or polls).  A group none of whose rows reported is finished: later rounds
 * walk only the rows of the groups that did report.
 * Cost, in the pass's current form: the rows are ALL N global rows whatever the context, divided in contiguous ranges over the
 * process's devices; every device holds all positions, gets the whole L and returns its rows' m.  In an nbody_init_rank job every rank
 * therefore walks all N rows on its own device and returns the same values: the call is collective only because the other slices'
 * positions are brought first, labels are not exchanged between processes, and P ranks do P times the work of one.
 * Like its siblings the call leaves positions, velocities, the arrival counters, the captured step graph and the force-kernel timer
 * as they were.
 * Environment, read on every call: NBODY_FOF_SPLIT = c >= 1 walks the sources in min(c, blocks of 1024) chunks side by side (unset or 0:
 * chosen from the number of active rows and the CU count); NBODY_FOF_SCRATCH_MB (default 256, fractions allowed) bounds the 4 bytes per
 * row and chunk a split launch stores, larger rounds go in consecutive batches of rows; NBODY_FOF_ALL_ROWS = 1 walks every row in every
 * round.  Same group and rounds in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched or written, for both outputs NULL, b2 NaN
 * or b2 < 0 (b2 = +inf is legal: every non-NaN body in one group); NBODY_ERR_STATE for the other precision's entry point or while the
 * mailbox is served. */
int nbody_fof(float b2, int *group, int *n_groups, int *rounds);
int nbody_fof_d(double b2, int *group, int *n_groups, int *rounds);

/* ---- radial counts, pair histogram: how many bodies lie in each shell of distance (not in the reference) ----
 * The sections above say who is nearest and who hangs together; this one says how many: a density profile around a body or a centre,
 * and the pair counts DD(r) of the whole system, from which the radial distribution function g(r) and the two-point correlation
 * function follow.  Queries, skip and d2 are exactly the neighbour pass's: in the context precision T, for every body j,
 *   dx = xj - x;  dy = yj - y;  dz = zj - z;   d2_j = fma(dx, dx, fma(dy, dy, dz * dz))
 * no softening, independent of NBODY_OPT_ARITH, every operation IEEE-exact.
 * EDGES: edges2 holds n_bins + 1 squared radii in T, 1 <= n_bins <= NBODY_HIST_MAX_BINS, no NaN, non-decreasing.  Equal neighbours
 * give an empty bin; edges2[n_bins] = +inf is legal.
 * THE STATEMENT OF RECORD IS CUMULATIVE: for a query,
 *   c_b = #{ non-skipped j : d2_j < edges2[b] }   and   counts[b] = c_(b+1) - c_b,
 * with non-decreasing edges the number of j with edges2[b] <= d2_j < edges2[b+1].  So a NaN d2_j is below nothing and is never
 * counted; a d2_j that overflowed to +inf is never counted either (it is not below +inf); a coincident distinct body (d2 = +0) falls
 * in the bin that holds 0.
 * nbody_radial_counts_rows(_d): the queries are the bodies themselves, each excluding itself; rows exactly as in nbody_forces_rows and
 *   nbody_neighbors_rows.  counts: n_rows x n_bins ints, row-major: bin b of query p at [p * n_bins + b], as nbody_knn lays out its lists.
 * nbody_radial_counts(_d): the queries are m caller points; points, skip and the division over the devices as in nbody_nearest.
 *   nbody_init_rank: every rank asks for its own points, m and n_bins may differ between ranks.
 * nbody_pair_histogram(_d): pairs[b] is the number of unordered pairs i < j of the whole system in bin b.  d2 is symmetric bit for bit
 *   (the section above), so pairs[b] is half the sum over all N rows of the rows form's counts[b], and that sum is even.  The per-row
 *   counts are int32, the totals 64-bit (N = 70 000 already has more than 2^31 pairs).  Every device or rank runs the rows pass over its
 *   own rows, in batches under the scratch bound below, and adds them on the device to n_bins 64-bit sums; the per-row counts never go
 *   to the host.  The sums are added in rank order and halved after the sum over the ranks (one rank's own sum may be odd: a pair
 *   across ranks is counted once per side).  In an nbody_init_rank job it is collective and every rank returns the same values.
 * The values depend on the N positions, the query, its skip and the edges alone — not on m, on where the query stands, on the launch
 * shape (NBODY_HIST_SPLIT, NBODY_HIST_LOOP below), on the arithmetic, on the force configuration or on the device or rank count.  A bin
 * that merges adjacent bins of a finer edge list holds their sum.  nbody_radial_counts* with edges2 = {0, nextafter(r2, +inf)} equals
 * the neighbour pass's count at r2, for finite r2 >= 0.  The sums are integer sums (the pair histogram's with integer atomics), exact
 * in every order: two calls return identical values.
 * All three bring the other slices' positions first (collective in nbody_init_rank contexts) and, like their siblings, leave positions,
 * velocities, the arrival counters, the captured step graph and the force-kernel timer as they were.
 * Environment, read on every call: NBODY_HIST_SPLIT = c >= 1 walks the sources in min(c, blocks of 1024) chunks side by side (unset or 0:
 * chosen from the number of queries and the CU count); NBODY_HIST_SCRATCH_MB (default 256, fractions allowed) bounds the n_bins * 4
 * bytes per query and chunk a split launch stores, larger calls go in consecutive batches of queries, and it bounds the per-row counts
 * of nbody_pair_histogram in the same way (never below one workgroup's 256 rows); NBODY_HIST_LOOP = 1 compares every pair with every
 * edge, 2 first takes the minimum of each aligned window of 64 sources and walks it with the counters only if some query of the wave
 * has a body below the last edge (unset: 2, and 1 where the last edge is +inf and no window can be left out).  Same values in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched or written, for a NULL output, edges2 or
 * points, n_bins < 1 or > NBODY_HIST_MAX_BINS, a NaN or a descending edge, a bad row range, m < 1 or a skip value outside [-1, N);
 * NBODY_ERR_STATE for the other precision's entry point or while the mailbox is served. */
#define NBODY_HIST_MAX_BINS 32
int nbody_radial_counts_rows(int first_row, int n_rows, const float *edges2, int n_bins, int *counts);
int nbody_radial_counts_rows_d(int first_row, int n_rows, const double *edges2, int n_bins, int *counts);
int nbody_radial_counts(const float *points, int m, const int *skip, const float *edges2, int n_bins, int *counts);
int nbody_radial_counts_d(const double *points, int m, const int *skip, const double *edges2, int n_bins, int *counts);
int nbody_pair_histogram(const float *edges2, int n_bins, long long *pairs);
int nbody_pair_histogram_d(const double *edges2, int n_bins, long long *pairs);

/* ---- pair time scales and a shared adaptive time step: how soon two bodies meet (not in the reference) ----
 * The first pass that reads two bodies' velocities together.  In the context precision T, for a row i and every body j != i:
 *   dx = xj - xi (dy, dz likewise)         d2 = fma(dx, dx, fma(dy, dy, dz * dz))     the neighbour pass's plain d2, unchanged
 *   ux = vxj - vxi (uy, uz likewise)       v2 = fma(ux, ux, fma(uy, uy, uz * uz))
 *   q  = d2 / v2                           the correctly rounded IEEE quotient: the pair crossing time squared
 * every operation IEEE-exact, contraction off, no softening, and none of it follows NBODY_OPT_ARITH: one definition per precision.
 *   tau2   the smallest q over j, in T.  A NaN q (0 / 0, a NaN anywhere) is never chosen, nor is q = +inf (v2 = 0 with d2 > 0, a d2
 *          that overflowed): it is not below +inf.  A v2 that overflows to +inf gives q = +0, a legitimate answer, as is the +0 of a
 *          coincident body that moves.
 *   idx    the j that gives it, on equal values the lowest j: what an ascending scan from (+inf, -1) that replaces on strict < arrives
 *          at.  Without a candidate (N = 1, every q NaN or +inf): idx = -1, tau2 = +inf.
 *   d2min  the smallest d2 over j, in T: bit for bit the d2 of nbody_neighbors_rows.  The other standard time scale, the pair free-fall
 *          time, is monotone in the distance and follows from it.
 * Minima are exact: the values depend on the N positions and velocities and the row alone — not on the number of rows, on the launch
 * shape (NBODY_TIMESCALE_SPLIT below), on the arithmetic, on the force configuration or on the device or rank count.  No atomics.
 * nbody_timescale_rows(_d): rows exactly as in nbody_forces_rows (nbody_init: first_row is a global index, the range may span devices;
 *   nbody_init_rank: a row of the rank's own slice).  The idx returned are always GLOBAL body indices.  tau2, idx or d2min may be NULL
 *   (at least one is not).
 * nbody_min_timescale(_d): the smallest tau2 of the whole system, i the lowest row that reaches it and j that row's partner, and the
 *   smallest d2min of the whole system (nbody_closest_pair's d2); -1, -1 and +inf where there is none.  Any of the four may be NULL
 *   (not all).  It runs the rows pass over every device's or rank's own rows and keeps each one's best by a fixed-order reduction; the
 *   winner is picked in rank order with strict <.  Every rank returns the same values.
 * All of them bring the other slices' positions first and then ALL N velocities to every device: one device reads its own; the devices
 * of an nbody_init context copy each other's slices device to device; an nbody_init_rank job gathers them with the transport it uses
 * for positions, so every call is collective there.  A diagnostic call pays for that.  They leave positions, velocities, the arrival
 * counters, the captured step graph and the force-kernel timer as they were.
 * nbody_step_adaptive(_d): a shared adaptive time step on top of nbody_step, from t = 0, everything but the step itself in binary64:
 *     (tau2, d2min) of nbody_min_timescale;  s = d2min + eps (the force's eps);  tff2 = s * sqrt(s) / 2  (the unit-mass pair free-fall
 *     time squared);  h = eta * sqrt(min(tau2, tff2));  h clamped to [dt_min, dt_max];  h = t_end - t if t + h > t_end;  dt = h rounded
 *     once to T;  one eager step of dt, exactly nbody_step(dt, 1);  t += (double)dt
 *   until t >= t_end or max_steps steps are taken (then NBODY_OK with *t_reached < t_end).  *t_reached and *steps_taken (either may be
 *   NULL) are written after every step.  dt_min > 0 is what keeps coincident bodies (tau2 = 0) from stalling it.  Every rank computes
 *   the same h from the same values: a multi-rank job needs no further exchange.
 * Environment, read on every call: NBODY_TIMESCALE_SPLIT = k >= 1 walks the sources in min(k, blocks of 1024) chunks side by side
 * (unset or 0: chosen from the number of rows and the CU count); NBODY_TIMESCALE_SCRATCH_MB (default 256, fractions allowed) bounds the
 * 12 (fp64: 20) bytes per row and chunk a split launch stores, larger calls go in consecutive batches of rows.  Same values in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched or written, for every output NULL, a bad row
 * range, a non-finite eta, t_end, dt_min or dt_max, eta <= 0, dt_min <= 0, dt_max < dt_min, t_end <= 0 or max_steps < 1;
 * NBODY_ERR_STATE for the other precision's entry point or while the mailbox is served.
 * nbody_timescale_rows and nbody_min_timescale are kinematics and do not follow NBODY_OPT_MASSES.  nbody_step_adaptive(_d) — its
 * free-fall time and its kick are unit-mass —: NBODY_ERR_UNSUPPORTED while NBODY_OPT_MASSES is 1 (unit masses only), before anything is launched, copied or written. */
int nbody_timescale_rows(int first_row, int n_rows, float *tau2, int *idx, float *d2min);
int nbody_timescale_rows_d(int first_row, int n_rows, double *tau2, int *idx, double *d2min);
int nbody_min_timescale(float *tau2, int *i, int *j, float *d2min);
int nbody_min_timescale_d(double *tau2, int *i, int *j, double *d2min);
int nbody_step_adaptive(float eta, float t_end, float dt_min, float dt_max, int max_steps, double *t_reached, int *steps_taken);
int nbody_step_adaptive_d(double eta, double t_end, double dt_min, double dt_max, int max_steps, double *t_reached, int *steps_taken);

/* ---- pair binding energies and binaries: which pairs are bound, and on what orbit (not in the reference) ----
 * Masses are unit and G = 1, so the relative orbit of a pair has mu = 2.  In the context precision T, for a row i and every body j != i:
 *   dx = xj - xi (dy, dz likewise)         d2 = fma(dx, dx, fma(dy, dy, dz * dz))     the neighbour pass's plain d2, unchanged
 *   ux = vxj - vxi (uy, uz likewise)       v2 = fma(ux, ux, fma(uy, uy, uz * uz))     the time-scale pass's v2, unchanged
 *   s  = d2 + eps                          eps the force's softening
 *   inv = 1 / sqrt(s)                      binary32: the value (float)(1.0 / sqrt((double)s)), the strict modes' 1/sqrt;
 *                                          binary64: the IEEE sqrt followed by the IEEE divide
 *   e  = fma((T)0.5, v2, (T)-2 * inv)      the specific orbital energy v^2 / 2 - mu / r of the softened pair, rounded once
 * every operation rounded once, contraction off, and none of it follows NBODY_OPT_ARITH: one definition per precision.  The softening
 * keeps coincident distinct bodies at the finite e = v2 / 2 - 2 / sqrt(eps) instead of -inf.
 *   e      the lowest e over j, in T.  A NaN e (a NaN coordinate anywhere in the pair) is never chosen, nor is e = +inf (a v2 that
 *          overflowed): it is not below +inf.  A d2 that overflows gives inv = +0 and e = v2 / 2, a legitimate non-negative candidate.
 *   idx    the j that gives it, on equal values the lowest j: what an ascending scan from (+inf, -1) that replaces on strict < arrives
 *          at.  Without a candidate (N = 1, every e NaN or +inf): idx = -1, e = +inf.
 * e_ij and e_ji have the same bits (the differences change sign, their squares do not).  A minimum of individually rounded values is
 * exact: the values depend on the N positions and velocities and the row alone — not on the number of rows, on the launch shape
 * (NBODY_PAIR_ENERGY_SPLIT below), on the arithmetic, on the force configuration or on the device or rank count.  No atomics: two calls
 * return identical values.
 * nbody_pair_energy_rows(_d): rows exactly as in nbody_timescale_rows (nbody_init: first_row is a global index, the range may span
 *   devices; nbody_init_rank: a row of the rank's own slice).  The idx returned are always GLOBAL body indices.  e or idx may be NULL
 *   (not both).  It brings the other slices' positions first and then ALL N velocities to every device, exactly as
 *   nbody_timescale_rows does, so it is collective in an nbody_init_rank job.
 * nbody_binaries (both precisions): the rows pass over all N global rows, then on the host, in ascending i, every pair i < j with
 *   idx[i] == j, idx[j] == i and e[i] < e_max: the mutually most bound pairs.  *n_pairs is the number found and may exceed max_pairs; the
 *   first min(*n_pairs, max_pairs) are written to i[k], j[k] and elements[NBODY_BINARY_WORDS * k ..] = {E, a, ecc, period}.  With
 *   max_pairs == 0 the three arrays may be NULL and the call only counts.  e_max <= 0; e_max = -inf is legal and lists nothing.  A body
 *   whose best partner prefers someone else is NOT listed — this is how a hierarchy shows: of a triple, only the inner pair is.
 *   The rows are divided in contiguous ranges over the process's devices; in an nbody_init_rank job every rank walks all N rows on its
 *   own device, as nbody_fof does — P times the work of one rank, paid for a list that is the same on every rank without an exchange
 *   beyond the gathers above (which keep the call collective).
 *   The elements are computed on the host in binary64 from the two members' T-valued state converted exactly, in this order:
 *     d = r_j - r_i;  u = v_j - v_i;  s = ((dx*dx + dy*dy) + dz*dz) + (double)eps;  r = sqrt(s);  v2 = (ux*ux + uy*uy) + uz*uz;
 *     E = 0.5*v2 - 2.0/r;  a = -1.0/E;  L2 = |d x u|^2 (c = d x u, (cx*cx + cy*cy) + cz*cz);  ecc = sqrt(max(0, 1 + (0.5*E)*L2));
 *     period = pi * sqrt(((2*a)*a)*a)
 *   Membership is decided by the T-valued e of the pass; the elements are a convenience.  A marginal pair may show E >= 0, and a and
 *   period are then what the formulas give (a negative a, a NaN period).
 * Both leave positions, velocities, the arrival counters, the captured step graph and the force-kernel timer as they were.
 * Environment, read on every call: NBODY_PAIR_ENERGY_SPLIT = k >= 1 walks the sources in min(k, blocks of 1024) chunks side by side
 * (unset or 0: chosen from the number of rows and the CU count); NBODY_PAIR_ENERGY_SCRATCH_MB (default 256, fractions allowed) bounds
 * the 8 (fp64: 12) bytes per row and chunk a split launch stores, larger calls go in consecutive batches of rows.  Same values in every case.
 * NBODY_ERR_NOT_INIT without a context; NBODY_ERR_ARG, checked before anything is launched or written, for a bad row range, both
 * outputs NULL, an e_max that is NaN or > 0, max_pairs < 0, n_pairs == NULL or a NULL array with max_pairs > 0; NBODY_ERR_STATE for the
 * other precision's rows entry point or while the mailbox is served.
 * nbody_pair_energy_rows(_d) and nbody_binaries (mu = 2): NBODY_ERR_UNSUPPORTED while NBODY_OPT_MASSES is 1 (unit masses only), before anything is launched, copied or written.
 * Mass-weighted pair energies and binaries (mu = m_i + m_j) are not built yet. */
#define NBODY_BINARY_WORDS 4
int nbody_pair_energy_rows(int first_row, int n_rows, float *e, int *idx);
int nbody_pair_energy_rows_d(int first_row, int n_rows, double *e, int *idx);
int nbody_binaries(double e_max, int max_pairs, int *n_pairs, int *i, int *j, double *elements);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_H */
