/*
 * ellhip_batch_lowpass_streamed_stable.h -- C ABI of the batched, device-resident low-pass filter design loop on a streamed
 * EllStable batch handle (libellhip.so).
 *
 * ellhip_batch_lowpass_streamed.h solves B independent `LowpassOracle` problems (src/oracles/lowpass_oracle.rs:7-151) of one
 * filter length n <= 1024 on streamed Ell spaces; ellhip_batch_stable_loops.h solves them on EllStable spaces of n <= 128
 * that fit in LDS.  This header fills the remaining cell: the spaces are a streamed EllStable batch handle
 * (ellhip_batch_streamed_stable.h: the packed buffers stay in HBM, one workgroup per ellipsoid, one thread per index) and one
 * kernel per chunk of iterations runs oracle, x_best, EllStable::update_core (src/ell_stable.rs:52-125) and the stop test
 * for every problem, no host in the loop.  Every step follows the reference's statement order, so cuts, iteration counts,
 * x_best, gamma, the oracle state and the spaces afterwards (the scratch triangle included) are bit-identical to the CPU
 * arithmetic and, at n <= 128, to ellhip_batch_lowpass_optim_stable / _feas_stable on an LDS handle.
 *
 * The oracle handle is an ordinary ellhip_batch_lowpass of either constructor (ellhip_batch_lowpass_create for n <= 128,
 * ellhip_batch_lowpass_create_streamed for n <= 1024); _set_chunk applies (256 iterations per launch by default).
 *
 * Traffic per problem and successful iteration: 24 n^2 bytes of packed buffer (no fusion across iterations: the centre of
 * iteration k is final only after its back solve, and the oracle of iteration k + 1 needs it), and for the oracle 8 n bytes
 * of table per row it visits plus 8 n for the gradient.  A failed cut moves 8 n^2 bytes and changes tsq and the scratch
 * triangle only, exactly as the CPU EllStable does.
 *
 * LDS per workgroup: 8 * (4 * (n rounded up to even) + 72 + ((n + 20) | 1)) bytes, 40.7 KiB at n = 1024.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_LOWPASS_STREAMED_STABLE_H
#define ELLHIP_BATCH_LOWPASS_STREAMED_STABLE_H

#include "ellhip_batch_lowpass_streamed.h"
#include "ellhip_batch_streamed_stable.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ellhip_batch_lowpass_optim_streamed on EllStable spaces: same arguments, semantics and outputs.  spaces must be a streamed
 * batch handle (ellhip_batch_is_streamed) of variant ELLHIP_SPACE_ELL_STABLE with the oracle's B, n and device; any
 * 1 <= n <= 1024 is accepted, n <= 128 included.  Anything else -- a streamed Ell handle, an LDS handle of either variant, a
 * mismatch, a NULL argument -- is ELLHIP_E_INVALID with a message, and the spaces and outputs are left untouched. */
int ellhip_batch_lowpass_optim_streamed_stable(ellhip_batch *spaces, ellhip_batch_lowpass *o, double *gamma_inout,
                                               int64_t max_iters, double tol, double *x_best_out, int32_t *has_best_out,
                                               int64_t *niter_out, int32_t *status_out);
/* ellhip_batch_lowpass_feas_streamed on EllStable spaces. */
int ellhip_batch_lowpass_feas_streamed_stable(ellhip_batch *spaces, ellhip_batch_lowpass *o, int64_t max_iters, double tol,
                                              double *x_out, int32_t *feasible_out, int64_t *niter_out,
                                              int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif
