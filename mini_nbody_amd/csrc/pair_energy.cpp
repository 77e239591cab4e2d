// pair_energy.cpp — nbody_pair_energy_rows(_d), nbody_binaries: per row the lowest specific two-body energy v2 / 2 - 2 / sqrt(d2 + eps)
// over the other bodies and the body that gives it (pair_energy.hip); and the binaries of the whole system, the mutually most bound
// pairs below an energy, with their osculating elements.  Host C++ only, in the shape of timescale.cpp.  Flow (query_pass.hpp):
// reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings them), all N velocities where every local's
// kernel can read them (gather_velocities), then per local its rows: the launch (and the combine launch when the sources are split)
// on the local's compute stream, stream sync, copy back.  nbody_binaries runs the rows pass over ALL N global rows whatever the
// context — contiguous ranges over the process's devices; in an nbody_init_rank job every rank walks them all on its own device, as
// nbody_fof does, and arrives at the same list — then the mutual test and the elements on the host, in binary64.
// The pass reads pos[cur] and vel and writes only the Local's q_scratch, pe_* buffers, ts_vel and (nbody_init_rank contexts)
// full_scratch: positions, velocities, arrival counters, partial forces, the captured step graph and the force-kernel timer stay as
// they were.  Nothing outside this file refers to it.
#include "query_pass.hpp"
#include "pair_energy_args.hpp"

#include <cmath>

#pragma STDC FP_CONTRACT OFF   // the elements are the operations include/nbody.h lists, each rounded once

using namespace nbpe;

namespace nbi {

namespace {

// Workgroups per CU a launch should have before its sources stop being split (query_pass.hpp's choose_chunks), in place of kQueryFill:
// the launch shape is the pair time-scale pass's and a pair costs more (a binary64 sqrt and divide in either precision), so one or two
// waves a SIMD hide as little.  Measured on 65 536 rows (tools/pair_energy_rate.py, profiles/r15_pair_energy.txt, medians of 7): 9.31 ms
// unsplit, 6.26 ms over 4 chunks, 5.58 ms over the 16 that kTimescaleFill would ask for, 5.43 ms over 32, 5.41 ms over 64 (fp64: 13.36,
// 7.54, 6.52, 6.33, 6.25): 32 is within 1.5 % of the best forced split in both precisions, 16 is 3 - 4 % behind it.
constexpr int kPairEnergyFill = 32;

// rows [first, first + cnt) of the SYSTEM (global indices) on L, with the outputs left at the start of pe_e / pe_idx for the copy back
int launch_pair_energy(Local& L, int first, int cnt, bool want_e, bool want_idx) {
  HIPC(hipSetDevice(L.device));
  const size_t es = elem_bytes();
  if (want_e) NBC(L.pe_e.ensure((size_t)cnt * es));
  if (want_idx) NBC(L.pe_idx.ensure((size_t)cnt * sizeof(int)));
  const int n_blocks = source_blocks();
  const SplitPlan plan = chunk_split("NBODY_PAIR_ENERGY_SPLIT", "NBODY_PAIR_ENERGY_SCRATCH_MB", cnt, n_blocks, pair_energy_scratch_bytes(1, 1, es),
                                     kPairEnergyFill);
  if (plan.chunks > 1) NBC(L.q_scratch.ensure(pair_energy_scratch_bytes((size_t)plan.batch, (size_t)plan.chunks, es)));
  return for_batches(cnt, plan, [&](int b0, int m) {
    PairEnergyArgs a;
    memset(&a, 0, sizeof(a));
    fill_sources(a, L, plan, n_blocks, m, first + b0);
    a.vsrc = velocities_of(L);
    a.e = want_e ? L.pe_e.as<char>() + (size_t)b0 * es : nullptr;
    a.idx = want_idx ? L.pe_idx.as<int>() + b0 : nullptr;
    a.scratch = plan.chunks > 1 ? L.q_scratch.as<void>() : nullptr;
    HIPC((hipError_t)nbl::launch_pair_energy_kernel(g.fp64, L.compute, a));
    if (plan.chunks > 1) HIPC((hipError_t)nbl::launch_pair_energy_combine_kernel(g.fp64, L.compute, a));
    return NBODY_OK;
  });
}

int rows_impl(int first_row, int n_rows, void* e, int* idx) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!e && !idx) return NBODY_ERR_ARG;
  RowWindow w;   // rows as in nbody_timescale_rows
  NBC(w.open(first_row, n_rows));
  NBC(reconfigure());
  NBC(complete_positions());
  NBC(gather_velocities());
  return run_on_locals([&](int l) { return rows_of(w, l); },
                       [&](Local& L, const Range& r) { return launch_pair_energy(L, L.first + r.first, r.cnt, e != nullptr, idx != nullptr); },
                       [&](Local& L, const Range& r) {
                         NBC(copy_out(e, r.out, L.pe_e, r.cnt, elem_bytes()));
                         return copy_out(idx, r.out, L.pe_idx, r.cnt, sizeof(int));
                       });
}

// member i's word of a downloaded state (context precision), converted exactly
struct Vec3 { double x, y, z; };
Vec3 word_of(const std::vector<char>& words, int i) {
  if (g.fp64) { const double* p = (const double*)words.data() + 4 * (size_t)i; return {p[0], p[1], p[2]}; }
  const float* p = (const float*)words.data() + 4 * (size_t)i;
  return {(double)p[0], (double)p[1], (double)p[2]};
}

// {E, a, ecc, period} of the pair (i, j): the operations of include/nbody.h in their order, binary64
void elements_of(const std::vector<char>& pos, const std::vector<char>& vel, int i, int j, double* out) {
  const Vec3 ri = word_of(pos, i), rj = word_of(pos, j), vi = word_of(vel, i), vj = word_of(vel, j);
  const double dx = rj.x - ri.x, dy = rj.y - ri.y, dz = rj.z - ri.z;
  const double ux = vj.x - vi.x, uy = vj.y - vi.y, uz = vj.z - vi.z;
  float eps32;
  memcpy(&eps32, &nbk::kSoftBits, sizeof(eps32));   // the force's eps
  const double s = ((dx * dx + dy * dy) + dz * dz) + (double)eps32;
  const double r = std::sqrt(s);
  const double v2 = (ux * ux + uy * uy) + uz * uz;
  const double E = 0.5 * v2 - 2.0 / r;
  const double a = -1.0 / E;
  const double cx = dy * uz - dz * uy, cy = dz * ux - dx * uz, cz = dx * uy - dy * ux;
  const double L2 = (cx * cx + cy * cy) + cz * cz;
  const double k = 1.0 + (0.5 * E) * L2;
  out[0] = E;
  out[1] = a;
  out[2] = std::sqrt(k > 0.0 ? k : 0.0);   // (a NaN k gives 0, as max(0, .) does)
  out[3] = 3.14159265358979323846 * std::sqrt(((2.0 * a) * a) * a);
}

int binaries_impl(double e_max, int max_pairs, int* n_pairs, int* pi, int* pj, double* elements) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!(e_max <= 0.0) || max_pairs < 0 || !n_pairs) return NBODY_ERR_ARG;   // (a NaN e_max is not <= 0)
  if (max_pairs > 0 && (!pi || !pj || !elements)) return NBODY_ERR_ARG;
  NBC(reconfigure());
  NBC(complete_positions());
  NBC(gather_velocities());
  const int n = g.n;
  const size_t es = elem_bytes(), wb = word_bytes();
  std::vector<char> e((size_t)n * es);
  std::vector<int> idx((size_t)n);
  NBC(run_on_locals([&](int l) { return points_of(n, l); },
                    [&](Local& L, const Range& r) { return launch_pair_energy(L, r.first, r.cnt, true, true); },
                    [&](Local& L, const Range& r) {
                      NBC(copy_out(e.data(), r.out, L.pe_e, r.cnt, es));
                      return copy_out(idx.data(), r.out, L.pe_idx, r.cnt, sizeof(int));
                    }));
  const auto e_of = [&](int i) { return g.fp64 ? ((const double*)e.data())[i] : (double)((const float*)e.data())[i]; };
  std::vector<int> found;   // the lower member of every mutual pair below e_max, ascending
  for (int i = 0; i < n; ++i) {
    const int j = idx[(size_t)i];
    if (j > i && j < n && idx[(size_t)j] == i && e_of(i) < e_max) found.push_back(i);
  }
  const int listed = std::min((int)found.size(), max_pairs);
  if (listed > 0) {   // the members' state as the pass read it: the first local's complete positions and all N velocities
    Local& L = g.loc[0];
    std::vector<char> pos((size_t)n * wb), vel((size_t)n * wb);
    HIPC(hipSetDevice(L.device));
    HIPC(hipStreamSynchronize(L.compute));
    HIPC(hipMemcpy(pos.data(), L.pos[L.cur], (size_t)n * wb, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(vel.data(), velocities_of(L), (size_t)n * wb, hipMemcpyDeviceToHost));
    for (int k = 0; k < listed; ++k) {
      const int i = found[(size_t)k], j = idx[(size_t)i];
      pi[k] = i;
      pj[k] = j;
      elements_of(pos, vel, i, j, elements + (size_t)NBODY_BINARY_WORDS * (size_t)k);
    }
  }
  *n_pairs = (int)found.size();
  return NBODY_OK;
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_pair_energy_rows(int first_row, int n_rows, float* e, int* idx) { NB_ENTER_UNIT_MASS(0);
  return rows_impl(first_row, n_rows, e, idx);
}
int nbody_pair_energy_rows_d(int first_row, int n_rows, double* e, int* idx) { NB_ENTER_UNIT_MASS(1);
  return rows_impl(first_row, n_rows, e, idx);
}
int nbody_binaries(double e_max, int max_pairs, int* n_pairs, int* i, int* j, double* elements) { NB_REFUSE_WHILE_SERVED(); NB_REFUSE_MASSES();
  return binaries_impl(e_max, max_pairs, n_pairs, i, j, elements);
}

}  // extern "C"
