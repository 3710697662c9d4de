// Test hook for the cone-local workgroup ids of csrc/polar_tiles.h (compiled by tests/test_polar_passes_host.py into its own shared object with g++):
// the functions the batch's populate-type kernels decode their workgroup id with.
#include "polar_tiles.h"

extern "C" {

int polar_passes_grid(int n, int bpx) { return polar_wg_grid(n, bpx); }
int polar_passes_id(int cone, int bx, int bpx) { return polar_wg_id(cone, bx, bpx); }
// out = {cone, bx}; cone == -1: none
void polar_passes_decode(int id, int n, int bpx, int out[2]) {
  const PolarWg w = polar_wg_decode(id, n, bpx);
  out[0] = w.cone; out[1] = w.bx;
}

}
