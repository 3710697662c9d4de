// host_csr.h -- host staging of a CSR matrix: the one definition that the HIP translation units (through internal.h) and the host-only ones
// (batch_image.cpp) share.  No HIP header.
#pragma once
#include <vector>
#include "../../include/cosmo_hip.h"

struct HostCsr {  // host staging of a CSR matrix (0-based)
  int nrows = 0, ncols = 0;
  std::vector<int> rowptr, col;
  std::vector<cosmo_hip_real> val;
  std::vector<int> split;
};
