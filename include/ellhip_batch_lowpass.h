/*
 * ellhip_batch_lowpass.h -- C ABI of the batched, device-resident cutting-plane loop for FIR low-pass filter design by
 * spectral factorisation (libellhip.so).
 *
 * B independent `LowpassOracle`s (src/oracles/lowpass_oracle.rs:7-151) of one filter length ndim = n <= 128: problem b
 * has its own band edges wpass[b] <= wstop[b] and ripple limits lp_sq[b], up_sq[b], sp_sq[b], its own three round-robin
 * cursors idx1 / idx2 / idx3, fmax / kmax and more_alt; the 15n x n table `spectrum` depends on n only and is shared.
 * nwpass = floor(wpass (15n - 1)) + 1 and nwstop = floor(wstop (15n - 1)) + 1 (:36-37).  A call visits the passband
 * rows, then the stopband rows, then the transition band, then the `x[0] < 0` station, each band in cyclic order after
 * its cursor, and answers with the cut of the first violated constraint (`assess_feas`, :58-133); `assess_optim`
 * (:139-150) sets sp_sq = gamma first and, where x is feasible, answers the objective cut (spectrum[kmax],
 * ParallelCut(0, Some(fmax))) with gamma = fmax.
 *
 * The loop entry points run `cutting_plane_optim` (src/cutting_plane.rs:286-313) or `cutting_plane_feas` (:205-227) for
 * every problem on the device: one workgroup-resident ellipsoid per problem (an ellhip_batch handle of `Ell` spaces),
 * oracle and update in the same kernel, no host in the loop.  Every row . x is the reference's left fold from 0.0 and
 * every beta the expression the reference writes, so cuts, iteration counts, x_best, gamma, the oracle state and the
 * spaces afterwards are bit-identical to the CPU arithmetic.  (The single-problem oracle of ellhip_lowpass.h sums a row
 * in another order and is close to 1e-12 only; it serves n in the thousands, this one sweeps of small problems.)
 *
 * `EllStable` batch handles belong to ellhip_batch_stable_loops.h: the loop entry points refuse them with ELLHIP_E_INVALID.
 *
 * LDS: a workgroup holds `epw` problems, epw as the batch engine chooses it for n (ellhip_batch.h).  With p(k) = k | 1
 * it needs
 *
 *     epw * 8 * ( ((n * p(n) + 2 n + 8) | 1)  +  ((n + 20) | 1) )   bytes,
 *
 * the first term being the batch engine's own (matrix, gradient, Q g, scalars), the second the oracle's (x and its
 * scalars); the table stays in HBM / L2 (two copies, 2 * 15 n^2 * 8 bytes: 240 KiB at n = 32, 3.75 MiB at n = 128).  A
 * shape that needs more than 159 KiB (the device's 160 KiB per workgroup less 1 KiB the kernel keeps for itself) is
 * refused by the loop entry points; every n <= 128 fits (n = 128: 132.2 KiB).
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_LOWPASS_H
#define ELLHIP_BATCH_LOWPASS_H

#include "ellhip_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellhip_batch_lowpass ellhip_batch_lowpass;

/* LowpassOracle::new(n, wpass[b], wstop[b], lp_sq[b], up_sq[b], sp_sq[b]) for b = 0..B-1 (:23-53).  `spectrum`: the
 * shared table, row-major (15 n) x n, or NULL to have it computed exactly as the reference does (host libm; the same
 * code as ellhip_lowpass_create).  ELLHIP_E_INVALID for B <= 0 or B > 2^24, n outside 1..128, wpass > wstop or band
 * edges outside 0..1 for any b. */
int ellhip_batch_lowpass_create(ellhip_batch_lowpass **out, int64_t B, int64_t n, const double *wpass,
                                const double *wstop, const double *lp_sq, const double *up_sq, const double *sp_sq,
                                const double *spectrum, int device);
void ellhip_batch_lowpass_destroy(ellhip_batch_lowpass *o);

/* assess_feas (:58-133) for every problem at x[B][n].  cut_out[b] = 1: Some((grad_out[b], ParallelCut(beta0[b],
 * has_beta1[b] ? Some(beta1[b]) : None))); 0 = None (x[b] is feasible; that problem's outputs are left untouched). */
int ellhip_batch_lowpass_assess_feas(ellhip_batch_lowpass *o, const double *x, double *grad_out, double *beta0,
                                     int32_t *has_beta1, double *beta1, int32_t *cut_out);
/* assess_optim (:139-150) for every problem; gamma_inout[B] is `sp_sq`, shrunk_out[B] the bool.  rc_out[b] = 1, or
 * ELLHIP_E_STATE where x[b] is feasible but no stopband row exists (the reference would panic; outputs untouched). */
int ellhip_batch_lowpass_assess_optim(ellhip_batch_lowpass *o, const double *x, double *gamma_inout, double *grad_out,
                                      double *beta0, int32_t *has_beta1, double *beta1, int32_t *shrunk_out,
                                      int32_t *rc_out);
/* The structs' public fields, as ellhip_lowpass_state: ints7[B][7] = {more_alt, idx1, idx2, idx3, kmax, nwpass,
 * nwstop}, doubles2[B][2] = {fmax, sp_sq}.  Either may be NULL. */
int ellhip_batch_lowpass_state(ellhip_batch_lowpass *o, int32_t *ints7, double *doubles2);
/* Cursors, fmax and kmax (and more_alt) as after new(); sp_sq stays as the last call left it. */
int ellhip_batch_lowpass_reset(ellhip_batch_lowpass *o);
/* The shared table, row-major (15 n) x n. */
int ellhip_batch_lowpass_get_spectrum(ellhip_batch_lowpass *o, double *out);

/* cutting_plane_optim (src/cutting_plane.rs:286-313) for every problem, on the device.  spaces: an Ell batch handle with
 * the same B, n, device.  gamma_inout[B]; x_best_out[B][n] (rows with has_best_out[b] == 0 untouched); niter_out[B];
 * status_out[B] = the CutStatus of the last update (Success when the tolerance or max_iters ended the loop).  A problem
 * whose centre is feasible while it has no stopband row stops with ELLHIP_UNKNOWN, its niter not advanced.  Afterwards
 * the spaces and the oracles are in the state the reference loop leaves them in (the update that hit the tolerance is
 * complete), so ellhip_batch_update, the getters and a second call continue from there. */
int ellhip_batch_lowpass_optim(ellhip_batch *spaces, ellhip_batch_lowpass *o, double *gamma_inout, int64_t max_iters,
                               double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                               int32_t *status_out);
/* cutting_plane_feas (src/cutting_plane.rs:205-227): x_out[b] = the first centre that assess_feas passes
 * (feasible_out[b] = 1, status Success), rows of the other problems untouched. */
int ellhip_batch_lowpass_feas(ellhip_batch *spaces, ellhip_batch_lowpass *o, int64_t max_iters, double tol,
                              double *x_out, int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);
/* iterations per launch (default 256, 1..4096): the host looks at the "all stopped" count between launches */
int ellhip_batch_lowpass_set_chunk(ellhip_batch_lowpass *o, int64_t iters);

#ifdef __cplusplus
}
#endif
#endif
