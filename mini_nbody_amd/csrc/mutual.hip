// mutual.hip — the mutual pairing of the fp32 force pass (NBODY_OPT_PAIRING = 2): every unordered pair evaluated
// once, the bits of the ordered pass.  One kernel and its launch function (mutual_args.hpp); compiled into the library's one code
// object through device.hip.  gfx950 only.
//
// mutual_pairs_f32: the 64 lanes of a wave are a systolic array.  The wave owns one row block A of 1024 bodies — lane l holds rows
// 16 l .. 16 l + 15 with their positions and their 16 x 3 level-1 accumulators in registers — and a stream of source bodies j enters at
// lane 0 and moves one lane per step (v_mov_b32_dpp wave_shr:1; the new source is the move's `old` operand, which lane 0 keeps).  With
// each source travel its position and its MIRRORED accumulator m_j, zero at lane 0.  Per step lane l evaluates the 16 pairs (row 16 l + r, j)
// once each, r ascending, and adds fma(d, inv3, a_r) to the row's accumulator (the direct side: sources arrive in ascending j) and
// fma(-d, inv3, m_j) to the travelling one (the mirrored side: row j meets the sources of A in ascending index — lanes ascend, rows
// within a lane ascend).  When j leaves lane 63, m_j IS the level-1 sum of row j over source block A.
// Same bits as the ordered pass (nbody_kernels.hpp, pair_f32 / Sums / walk_blocks): x_i - x_j is exactly -(x_j - x_i); the d2 chain sees
// only squares; inv, inv2, inv3 are the same values; an accumulator that starts at +0 and adds products of finite terms never holds -0,
// so fma(-d, inv3, m) is the fma the ordered kernel issues for row j — up to the sign and payload of a NaN (the mirrored side negates
// with the operand modifier, not with a second subtraction).
// A lane meets a block boundary of the stream l steps after lane 0: there it writes its 16 finished direct sums (256 contiguous bytes) to
// T[source block][its rows] and zeroes them — exec-masked code behind a branch that is skipped when no lane is at a boundary (64 steps
// in 1024).  Lane 63 stores the leaving m_j (16 bytes) every step to T[A][row j].  Lanes outside the stream (the first 63 steps of a unit
// and the 63 after its last source) are masked off.  No LDS, no barrier: the waves of a workgroup take different units.
// The rows are finished inside the same launch: a unit counts the table words it has written on a counter per row block, and the wave
// that completes a row block's nb words folds its 1024 rows (count_words, fold_row) — one launch per step, as the ordered pass.
#include <hip/hip_runtime.h>

#include "mutual_args.hpp"
#include "nbody_kernels.hpp"

using namespace nbk;

#define NBM_HIDDEN __attribute__((visibility("hidden")))

namespace nbm {

// v_mov_b32_dpp dst, src wave_shr:1 with dst = fresh beforehand: lane l takes lane l - 1's src across the whole wave (rows of 16 lanes
// included), lane 0 — which has no source lane — keeps `fresh`
__device__ __forceinline__ float shift_in(float fresh, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fresh), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

// One unit: row block A against the `count` source blocks A + d0, A + d0 + 1, ... (mod nb).  d0 = 0 is the diagonal unit (one block):
// ordered evaluation of block A against itself, the self pair included — the same code with the mirrored sums never stored (1 / nb of
// the work pays three fma per pair for nothing; a second form of the loop would double the kernel and spill across the two).
__device__ __forceinline__ void run_unit(const MutualArgs& a, const int A, const int d0, const int count, const int lane) {
  const float eps = soft_f32();
  const NB_CONST f4* src = (const NB_CONST f4*)(uintptr_t)a.src;
  const int row0 = A * kBlock + kRowsPerLane * lane;   // this lane's first row
  float xi[kRowsPerLane], yi[kRowsPerLane], zi[kRowsPerLane], ax[kRowsPerLane], ay[kRowsPerLane], az[kRowsPerLane];
  {
    const f4* rows = (const f4*)a.src + row0;
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
      const f4 w = rows[r];
      xi[r] = w.x; yi[r] = w.y; zi[r] = w.z;
      asm volatile("" : "+v"(xi[r]), "+v"(yi[r]), "+v"(zi[r]));   // three registers of their own: the loaded word's tuple, w included, would stay live
      ax[r] = 0.0f; ay[r] = 0.0f; az[r] = 0.0f;
    }
  }
  const int first = A + d0 < a.nb ? A + d0 : A + d0 - a.nb;   // the unit's first source block
  const int S = count * kBlock;                                // sources in the stream
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, mx = 0.0f, my = 0.0f, mz = 0.0f;   // the source this lane holds and its mirrored sums
  int s = -lane - 1;                                           // its index in the stream, once incremented: step t - lane
  unsigned moff = (unsigned)(first * kBlock - lane - 1);       // ... and its row, i.e. its word in T[A] (wraps while s < 0: never used then)
  f4* const t_mirror = a.table + (size_t)A * (size_t)a.n;
  // one step: shift the stream by one lane, inject p at lane 0, evaluate, flush what is finished
  auto step = [&](const f4 p) __attribute__((always_inline)) {
    sx = shift_in(p.x, sx); sy = shift_in(p.y, sy); sz = shift_in(p.z, sz);
    mx = shift_in(0.0f, mx); my = shift_in(0.0f, my); mz = shift_in(0.0f, mz);
    s += 1; moff += 1u;
    if ((unsigned)s < (unsigned)S) {
#pragma unroll
      for (int r = 0; r < kRowsPerLane; ++r) {
        // pair_f32<0>'s expressions in pair_f32<0>'s order, with d and inv3 kept for the second side
        const float dx = sx - xi[r];
        const float dy = sy - yi[r];
        const float dz = sz - zi[r];
        const float d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, eps)));
        const float inv = __builtin_amdgcn_rsqf(d2);
        const float inv2 = inv * inv;
        const float inv3 = inv * inv2;
        ax[r] = __builtin_fmaf(dx, inv3, ax[r]);
        ay[r] = __builtin_fmaf(dy, inv3, ay[r]);
        az[r] = __builtin_fmaf(dz, inv3, az[r]);
        // used here: without it the compiler sinks the 48 direct fma to the end of the step, behind the mirrored chain, and keeps d and
        // inv3 of all sixteen pairs alive (64 registers, spilled)
        asm volatile("" : "+v"(ax[r]), "+v"(ay[r]), "+v"(az[r]));
        mx = __builtin_fmaf(-dx, inv3, mx);
        my = __builtin_fmaf(-dy, inv3, my);
        mz = __builtin_fmaf(-dz, inv3, mz);
      }
      if (lane == 63 && d0 != 0) { const f4 o = {mx, my, mz, 0.0f}; t_mirror[moff] = o; }
      if ((s & (kBlock - 1)) == kBlock - 1) {   // this lane has seen the last source of a block: its 16 direct sums are finished
        int blk = first + (s >> 10);
        if (blk >= a.nb) blk -= a.nb;
        int l = lane;
        asm volatile("" : "+v"(l));   // the address is made here, not kept in two registers through the loop
        f4* out = a.table + (size_t)blk * (size_t)a.n + (A * kBlock + kRowsPerLane * l);
#pragma unroll
        for (int r = 0; r < kRowsPerLane; ++r) {
          float ox = ax[r], oy = ay[r], oz = az[r];
          asm volatile("" : "+v"(ox), "+v"(oy), "+v"(oz));   // copies: the accumulators themselves must not be allocated as 4-register store tuples
          const f4 o = {ox, oy, oz, 0.0f};
          out[r] = o;
          ax[r] = 0.0f; ay[r] = 0.0f; az[r] = 0.0f;
        }
        int nxt = blk + 1;
        if (nxt >= a.nb) nxt -= a.nb;
        moff = (unsigned)(nxt * kBlock) - 1u;     // the next source this lane takes is the first of block nxt
      }
    }
  };
  // the stream, block by block, then 64 more steps that push the last sources through the array (what is injected then is never used:
  // the first words of the source array, which exist)
  constexpr int G = 4;   // sources per scalar-load group: one s_load_dwordx16
  for (int bi = 0; bi <= count; ++bi) {
    int blk = first + bi;
    if (blk >= a.nb) blk -= a.nb;
    const int base = bi < count ? blk * kBlock : 0;
    const int len = bi < count ? kBlock : 64;
    f4 cur[G];
#pragma unroll
    for (int k = 0; k < G; ++k) cur[k] = src[base + k];
    for (int j = 0; j < len; j += G) {
      const int jn = j + G < len ? j + G : j;   // the group after the last: the last again, unused
      f4 nxt[G];
#pragma unroll
      for (int k = 0; k < G; ++k) nxt[k] = src[base + jn + k];
#pragma unroll
      for (int k = 0; k < G; ++k) step(cur[k]);
#pragma unroll
      for (int k = 0; k < G; ++k) cur[k] = nxt[k];
    }
  }
}

// Levels 2-4 of the ordered sum of row i on the table, in the ordered pass's own words: per piece b = 0, then b = b + T[blk][i] over
// the piece's blocks ascending (Sums::fold); the pieces of a segment joined piece 0 + piece 1 + ... (finish_rows, WS > 1); the segments
// joined ascending, the first by assignment (finish_rows, kFinishLast); apply_force.  Every piece boundary is a multiple of 1024 (the
// host checks it), so a block belongs to exactly one piece.
__device__ __forceinline__ void fold_row(const MutualArgs& a, const int i) {
  const f4* col = a.table + i;
  const size_t stride = (size_t)a.f.n_src;
  float fx = 0.0f, fy = 0.0f, fz = 0.0f;
  for (int q = 0; q < a.f.nslices; ++q) {
    for (int t = 0; t < a.f.sub; ++t) {
      int jb, je;
      segment_bounds(q, t, a.f.n_src, a.f.nslices, a.f.sub, &jb, &je);
      float sx = 0.0f, sy = 0.0f, sz = 0.0f;
      for (int w = 0; w < a.f.wsplit; ++w) {
        int pb = jb, pe = je;
        if (a.f.wsplit > 1) piece_bounds(jb, je, w, a.f.wsplit, &pb, &pe);
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        int blk = pb >> 10;
        const int end = pe >> 10;
        constexpr int F = 16;   // table words in flight per row
        for (; blk + F <= end; blk += F) {
          f4 e[F];
#pragma unroll
          for (int k = 0; k < F; ++k) e[k] = col[(size_t)(blk + k) * stride];
#pragma unroll
          for (int k = 0; k < F; ++k) { bx = bx + e[k].x; by = by + e[k].y; bz = bz + e[k].z; }
        }
        for (; blk < end; ++blk) {
          const f4 e = col[(size_t)blk * stride];
          bx = bx + e.x; by = by + e.y; bz = bz + e.z;
        }
        if (w == 0) { sx = bx; sy = by; sz = bz; }
        else { sx = sx + bx; sy = sy + by; sz = sz + bz; }
      }
      if (q == 0 && t == 0) { fx = sx; fy = sy; fz = sz; }
      else { fx = fx + sx; fy = fy + sy; fz = fz + sz; }
    }
  }
  const f4 me = ((const f4*)a.f.rows)[i];
  apply_force<float, f4>(a.f, i, me, fx, fy, fz);
}

// `words` more table words of row block X are written.  A row block has nb of them, one per source block; the wave that brings the
// count to nb — whichever it is — folds the block's 1024 rows (consecutive lanes, consecutive rows: coalesced) and zeroes the count for
// the next pass.  The hand-off is the one of finish_rows (nbody_kernels.hpp, kFinishLast): the caller has released its own words at
// agent scope before the first count, the count is an agent-scope atomic performed at memory, and the last arriver acquires at agent
// scope before it reads the table.  Nothing ever waits on another wave.
__device__ __forceinline__ void count_words(const MutualArgs& a, const int X, const int words, const int lane) {
  unsigned before = 0;
  if (lane == 0) before = __hip_atomic_fetch_add(a.tickets + X, (unsigned)words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  before = (unsigned)__builtin_amdgcn_readfirstlane((int)before);
  if (before + (unsigned)words != (unsigned)a.nb) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  for (int k = 0; k < kBlock / 64; ++k) fold_row(a, X * kBlock + k * 64 + lane);
  if (lane == 0) __hip_atomic_store(a.tickets + X, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 128 VGPRs at most: four waves per SIMD
__global__ void __launch_bounds__(64 * kWavesPerWg, 4) mutual_pairs_f32(MutualArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int u = (int)blockIdx.x * kWavesPerWg + wave;
  if (u >= a.nunits) return;
  const Unit un = mutual_unit(a.nb, a.run, u);
  if (un.count <= 0) return;
  run_unit(a, un.a, un.d0, un.count, lane);
  // the unit's words are in the table: `count` of row block A's (one, the diagonal unit's) and one of every partner's
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  count_words(a, un.a, un.count, lane);
  if (un.d0 != 0) {
    for (int k = 0; k < un.count; ++k) {
      int X = un.a + un.d0 + k;
      if (X >= a.nb) X -= a.nb;
      count_words(a, X, 1, lane);
    }
  }
}

}  // namespace nbm

namespace nbl {

NBM_HIDDEN int launch_mutual_pairs_kernel(hipStream_t st, const nbm::MutualArgs& a) {
  const int wgs = (a.nunits + nbm::kWavesPerWg - 1) / nbm::kWavesPerWg;
  hipLaunchKernelGGL(nbm::mutual_pairs_f32, dim3(wgs), dim3(64 * nbm::kWavesPerWg), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace nbl
