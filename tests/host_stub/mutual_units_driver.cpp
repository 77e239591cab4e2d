// mutual_units_driver.cpp — TEST INFRASTRUCTURE (tests/test_mutual_units.py): prints the work units of the mutual pairing as the library's
// own host/device function enumerates them (csrc/mutual_args.hpp: mutual_units, mutual_unit).  One line per unit: "nb run u a d0 count".
#include <stdio.h>
#include <stdlib.h>

#include "../../mini_nbody_amd/csrc/mutual_args.hpp"

int main(int argc, char** argv) {
  const int nb_max = argc > 1 ? atoi(argv[1]) : 40;
  for (int argi = 2; argi < argc; ++argi) {
    const int run = atoi(argv[argi]);
    for (int nb = 1; nb <= nb_max; ++nb) {
      const int units = nbm::mutual_units(nb, run);
      for (int u = 0; u < units; ++u) {
        const nbm::Unit un = nbm::mutual_unit(nb, run, u);
        printf("%d %d %d %d %d %d\n", nb, run, u, un.a, un.d0, un.count);
      }
    }
  }
  return 0;
}
