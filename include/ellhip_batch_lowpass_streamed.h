/*
 * ellhip_batch_lowpass_streamed.h -- C ABI of the batched, device-resident low-pass filter design loop on a streamed batch
 * handle (libellhip.so).
 *
 * ellhip_batch_lowpass.h solves B independent `LowpassOracle` problems (src/oracles/lowpass_oracle.rs:7-151) of one filter
 * length n <= 128 on the batch engine that keeps each matrix in LDS.  This header carries the same solve to n <= 1024: the
 * spaces are a streamed batch handle (ellhip_batch_streamed.h: the matrices stay in HBM, one workgroup per ellipsoid, one
 * thread per row) and one kernel per chunk of iterations runs oracle, scalar stage, centre, stop test and rank-1 update
 * for every problem, no host in the loop.  Every step follows the reference's statement order, so cuts, iteration counts,
 * x_best, gamma, the oracle state and the spaces afterwards are bit-identical to the CPU arithmetic and, at n <= 128, to
 * ellhip_batch_lowpass_optim / _feas on an LDS handle.
 *
 * The oracle handle is an ordinary ellhip_batch_lowpass: _destroy, _assess_feas, _assess_optim, _state, _reset,
 * _get_spectrum and _set_chunk of ellhip_batch_lowpass.h work on it at every n.  The table is kept in two layouts (row-major
 * for the gradient, transposed for the folds), 2 * 15 n^2 * 8 bytes in HBM: 3.75 MiB at n = 128, 60 MiB at n = 512, 240 MiB
 * at n = 1024, shared by all B problems.
 *
 * Traffic per problem for a launch of K successful iterations: (16 K + 8) n^2 bytes of matrix (the product of iteration
 * k + 1 rides on the update sweep of iteration k, because the oracle is called at the new centre before the sweep starts),
 * and for the oracle 8 n bytes of table per row it visits plus 8 n for the gradient.  At these n one step of the oracle's
 * walk (n rows) reads as many bytes as a matrix pass, so the oracle, not the update, sets the rate.
 *
 * LDS per workgroup: 8 * (5 * (n rounded up to even) + 8 + ((n + 20) | 1)) bytes, 48.2 KiB at n = 1024.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_LOWPASS_STREAMED_H
#define ELLHIP_BATCH_LOWPASS_STREAMED_H

#include "ellhip_batch_lowpass.h"
#include "ellhip_batch_streamed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ellhip_batch_lowpass_create for 1 <= n <= 1024 (ELLHIP_BATCH_STREAMED_NMAX); every other argument and refusal as there. */
int ellhip_batch_lowpass_create_streamed(ellhip_batch_lowpass **out, int64_t B, int64_t n, const double *wpass,
                                         const double *wstop, const double *lp_sq, const double *up_sq,
                                         const double *sp_sq, const double *spectrum, int device);

/* ellhip_batch_lowpass_optim on a streamed handle: same arguments, semantics and outputs.  spaces must be a streamed batch
 * handle (ellhip_batch_is_streamed) of Ell spaces with the oracle's B, n and device; a streamed handle of n <= 128 is
 * accepted.  Anything else is ELLHIP_E_INVALID with a message, and the spaces are left untouched. */
int ellhip_batch_lowpass_optim_streamed(ellhip_batch *spaces, ellhip_batch_lowpass *o, double *gamma_inout,
                                        int64_t max_iters, double tol, double *x_best_out, int32_t *has_best_out,
                                        int64_t *niter_out, int32_t *status_out);
/* ellhip_batch_lowpass_feas on a streamed handle. */
int ellhip_batch_lowpass_feas_streamed(ellhip_batch *spaces, ellhip_batch_lowpass *o, int64_t max_iters, double tol,
                                       double *x_out, int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif
