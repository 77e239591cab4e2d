// energy.cpp — nbody_energy and nbody_potential_rows(_d): the energy pass (energy.hip) over the state on the device.  Host C++ only.
// Flow (query_pass.hpp): reconfigure(), complete_positions() (the other slices, as nbody_forces_rows brings them), one pass per local
// on its compute stream, then the ranks' eight fp64 values added in rank order.  Processes exchange those values through the transport
// they use for positions (gather_rank_words), never a reduction, so every rank adds the same numbers in the same order.
// The pass reads pos[cur] and vel and writes only the Local's en_* buffers: positions, velocities, arrival counters, partial forces,
// the captured step graph and the force-kernel timer stay as they were.
#include "query_pass.hpp"
#include "energy_args.hpp"

using namespace nbe;

namespace nbi {

namespace {

int ensure_energy_buffers(Local& L) {
  HIPC(hipSetDevice(L.device));
  const size_t groups = ((size_t)L.n_local + kEnergyRows - 1) / kEnergyRows;
  NBC(L.en_part.ensure((groups + 1) * kEnergyWords * sizeof(double)));
  NBC(L.en_tot.ensure((size_t)g.nranks * kEnergyWords * sizeof(double)));
  return L.en_phi.ensure(((size_t)L.n_local + 1) * sizeof(double));
}

// rows [row0, row0 + row_count) of local L: phi into en_phi (totals = false) or the per-workgroup partials into en_part and their
// sum into word `rank` of en_tot (totals = true)
int launch_energy(Local& L, int row0, int row_count, bool totals) {
  NBC(ensure_energy_buffers(L));
  EnergyArgs a;
  memset(&a, 0, sizeof(a));
  a.src = L.pos[L.cur];
  a.vel = totals ? L.vel.as<void>() : nullptr;
  a.phi = totals ? nullptr : L.en_phi.as<void>();
  a.part = totals ? L.en_part.as<double>() : nullptr;
  a.n_src = g.n;
  a.first = L.first;
  a.row0 = row0;
  a.row_count = row_count;
  a.masses = g.opt.masses;
  HIPC((hipError_t)nbl::launch_energy_kernel(g.fp64, g.opt.arith, L.compute, a));
  if (totals) {
    const int groups = (row_count + kEnergyRows - 1) / kEnergyRows;
    HIPC((hipError_t)nbl::launch_energy_reduce_kernel(L.compute, L.en_part.as<double>(), groups, L.en_tot.as<double>() + (size_t)L.rank * kEnergyWords));
  }
  return NBODY_OK;
}

int energy_impl(double* out) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!out) return NBODY_ERR_ARG;
  NBC(reconfigure());
  NBC(complete_positions());
  for (int l = 0; l < g.nlocal; ++l) NBC(launch_energy(g.loc[l], 0, g.loc[l].n_local, true));
  std::vector<double> all((size_t)g.nranks * kEnergyWords, 0.0);
  NBC(gather_rank_words(&Local::en_tot, all.data(), kEnergyWords * (int)sizeof(double)));
  for (int q = 0; q < kEnergyWords; ++q) {
    double s = 0.0;
    for (int r = 0; r < g.nranks; ++r) s += all[(size_t)r * kEnergyWords + q];   // rank order
    out[q] = s;
  }
  return NBODY_OK;
}

int potential_rows_impl(int first_row, int n_rows, void* phi) {
  if (!g.init) return NBODY_ERR_NOT_INIT;
  if (!phi) return NBODY_ERR_ARG;
  RowWindow w;   // rows as in nbody_forces_rows
  NBC(w.open(first_row, n_rows));
  NBC(reconfigure());
  NBC(complete_positions());
  return run_on_locals([&](int l) { return rows_of(w, l); }, [&](Local& L, const Range& r) { return launch_energy(L, r.first, r.cnt, false); },
                       [&](Local& L, const Range& r) { return copy_out(phi, r.out, L.en_phi, r.cnt, elem_bytes()); });
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

int nbody_energy(double* out) { NB_REFUSE_WHILE_SERVED(); return energy_impl(out); }
int nbody_potential_rows(int first_row, int n_rows, float* phi) { NB_ENTER(0);
  return potential_rows_impl(first_row, n_rows, phi);
}
int nbody_potential_rows_d(int first_row, int n_rows, double* phi) { NB_ENTER(1);
  return potential_rows_impl(first_row, n_rows, phi);
}

}  // extern "C"
