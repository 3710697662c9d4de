// batch_devio.h -- device-memory inputs and results of a finalised batch (batch_devio.hip): the caller's q / b, warm-start iterates and the unscaled
// solution move between the caller's device arrays and the batch's own without a host copy (cosmo_hip_batch_update_qb_device,
// cosmo_hip_batch_set_iterates_device, cosmo_hip_batch_get_solution_device in batch.hip).  The launchers take raw device pointers and a stream, check
// nothing and never synchronise; they return hipGetLastError() of their launches.
#pragma once
#include "internal.h"

// A member list travels in the kernel arguments, BDEVIO_CHUNK entries per launch: no device buffer that a later call could overwrite while an earlier
// launch is still queued, and no copy that the host would have to wait for.
#define BDEVIO_CHUNK 256

// update!(model; q, b) of `count` members from device arrays.  q_raw: count * n or null, b_raw: count * m or null (both raw, unscaled).  members: HOST
// array of count indices into the batch (validated by the caller: in range, no duplicates), or null = members 0 .. count-1 in order.  Writes q, b, cls
// of the listed members exactly as k_batch_update_qb (batch.hip) does.
hipError_t bdevio_update_qb(hipStream_t st, int n, int m, int count, const int64_t* members, const real* q_raw, const real* b_raw, const real* Dsc,
                            const real* Esc, const real* csc, const unsigned char* nonneg, real big, real* q, real* b, int* cls);

// scale_variables! (src/scaling.jl:118-123) of the caller's unscaled x0 (nprob * n), s0, y0 (nprob * m; null = zeros), then w = [x; mu ./ rho + s],
// w_prev = w and s as k_batch_set_w (batch.hip) forms them.
hipError_t bdevio_set_iterates(hipStream_t st, int nprob, int n, int m, const real* x0, const real* s0, const real* y0, const real* Dinv, const real* Esc,
                               const real* Einv, const real* csc, const real* rho, real* w, real* w_prev, real* s);

// reverse_scaling! (src/scaling.jl:170-179) of the batch's iterates into the caller's x (nprob * n), s, y (nprob * m); any of them may be null.
hipError_t bdevio_export_solution(hipStream_t st, int nprob, int n, int m, const real* w_prev, const real* s, const real* mu, const real* Dsc,
                                  const real* Esc, const real* Einv, const real* cinv, real* x_out, real* s_out, real* y_out);
