// batch_ruiz.h -- modified Ruiz equilibration (scale_ruiz!, src/scaling.jl:21-116) of every member of a batch in ONE launch (batch_ruiz.hip), run on
// the host staging of batch.hip between cosmo_hip_batch_set_problem / set_cones and cosmo_hip_batch_set_params (cosmo_hip_batch_scale_ruiz).
#pragma once
#include <string>
#include <vector>
#include "internal.h"

// The batch's staging, by reference: the three CSR copies per member (A, A', merged [P | A'] rows with the split at the end of the P part), the
// concatenated vectors (member-major) and where the scaling goes.  skip[k] != 0: member k already carries a caller's scaling and is left as it is.
struct BRuizStage {
  int nprob = 0, nbox = 0;
  long long n = 0, m = 0;
  std::vector<HostCsr>*A = nullptr, *AT = nullptr, *PT = nullptr;
  std::vector<real>*q = nullptr, *b = nullptr, *box_l = nullptr, *box_u = nullptr;
  std::vector<real>*D = nullptr, *E = nullptr, *Dinv = nullptr, *Einv = nullptr, *c = nullptr, *cinv = nullptr;
  const ConeTable* cones = nullptr;
  const std::vector<char>* skip = nullptr;
};

// Upload, one launch (one workgroup per member), one copy back into the staging.  info = {work vectors: 0 LDS / 1 global slab, dynamic LDS bytes of
// the launch, members scaled, rounds}.  Returns COSMO_HIP_OK or COSMO_HIP_ERR_HIP (err says which call).
int32_t bruiz_run(BRuizStage& S, hipStream_t st, long long iterations, real min_scaling, real max_scaling, int64_t info[4], std::string& err);
