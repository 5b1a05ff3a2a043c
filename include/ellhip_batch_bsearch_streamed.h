/*
 * ellhip_batch_bsearch_streamed.h -- C ABI of the batched linear feasibility loops and of the batched, device-resident
 * bsearch on streamed batch handles (libellhip.so).
 *
 * ellhip_batch_bsearch.h runs the linear feasibility family with a movable target (MyOracle3, src/example3.rs, as a family)
 * and bsearch over BSearchAdaptor (src/cutting_plane.rs:403-419, :441-466) on the batch engines that keep each matrix in
 * LDS, so it stops at n = 128.  This header carries both to n <= 1024: the spaces are a streamed batch handle
 * (ellhip_batch_streamed.h for Ell, ellhip_batch_streamed_stable.h for EllStable: the matrices stay in HBM, one workgroup per
 * problem, one thread per row).  The oracle is the device function ellhip_batch_bsearch.h runs, with the same folds, the same
 * cursor and the same answers; feasible, niter, upper, rounds, ends, the cursors, the targets and the centres are
 * bit-identical to the CPU arithmetic and, at n <= 128, to the LDS entry points on an LDS handle.
 *
 * The oracle handle is an ordinary ellhip_batch_linfeas: _destroy, _set_chunk, _set_target, _state and _assess_feas of
 * ellhip_batch_bsearch.h work on it at every n (past n = 128 _assess_feas runs one workgroup of n threads, rounded up to
 * whole waves, per problem).  A handle made here with n <= 128 may also be given to the LDS entry points; an (n, J) whose
 * LDS block does not fit beside the LDS engines' matrices is refused there at call time.
 *
 * The clone of a probe (:410).  The batch handle's matrix, kappa and tsq (and, on Ell, its symmetry flag) are never written;
 * only xc is, by set_xc (:414).  The probe's space lives in buffers of the oracle handle, allocated by the first bsearch call
 * (8 (n^2 + n + 2) bytes per problem, with 136 bytes of bisection state).
 *
 *     Ell        The clone is a read.  A probe takes its products from the handle's matrix until its first successful cut;
 *                that cut's rank-1 sweep reads the handle's matrix and writes the probe buffer, and the probe goes on in
 *                the buffer.  A probe that is feasible at once, or whose first cut fails, moves no matrix bytes for the
 *                clone; a probe of K successful cuts moves what K cuts of ellhip_batch_linfeas_feas_streamed move (16 n^2
 *                bytes per cut with the next round's product riding on the sweep, 8 n^2 more for the first of a launch).
 *                The sweep of a probe's last cut is skipped.
 *     EllStable  The clone is a copy of the packed buffer, 16 n^2 bytes, made by the workgroup right before the probe's
 *                first cut (EllStable::update_core writes its scratch triangle even when the cut fails); a probe that is
 *                feasible at once copies nothing.  A cut moves 24 n^2 bytes, a failed one 8 n^2.
 *
 * A launch runs at most `chunk` rounds (a round is one oracle call), and a launch boundary may fall anywhere inside a probe.
 *
 * LDS per workgroup, with e(n) = n rounded up to even: the streamed engine's arrays (Ell 8 (5 e(n) + 8) bytes, EllStable
 * 8 (4 e(n) + 72)), the oracle's block 8 ((n + J + 9) | 1) and 136 bytes of state: at most 80.3 KiB (n = 1024, J = 4096),
 * inside what a workgroup has, so no (n, J) within the limits is refused by the streamed entry points.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_BSEARCH_STREAMED_H
#define ELLHIP_BATCH_BSEARCH_STREAMED_H

#include "ellhip_batch_bsearch.h"
#include "ellhip_batch_streamed.h"
#include "ellhip_batch_streamed_stable.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ELLHIP_BATCH_LINFEAS_STREAMED_JMAX 4096

/* ellhip_batch_linfeas_create for 1 <= n <= ELLHIP_BATCH_STREAMED_NMAX (1024) and 1 <= J <=
 * ELLHIP_BATCH_LINFEAS_STREAMED_JMAX (4096); every other argument and refusal as there, checked before the device is looked
 * for.  The same handle type: destroy it with ellhip_batch_linfeas_destroy. */
int ellhip_batch_linfeas_create_streamed(ellhip_batch_linfeas **out, int64_t B, int64_t n, int64_t J, const double *a,
                                         const double *c, int32_t shared, int device);

/* ellhip_batch_linfeas_feas on a streamed handle: same arguments, semantics and outputs.  spaces must be a streamed batch
 * handle (ellhip_batch_is_streamed) of Ell (_streamed) or EllStable (_streamed_stable) spaces with the oracle's B, n and
 * device; a streamed handle of n <= 128 is accepted.  Anything else -- an LDS handle, the other variant, a mismatch, a NULL
 * argument -- is ELLHIP_E_INVALID with a message, and the spaces and outputs are left untouched. */
int ellhip_batch_linfeas_feas_streamed(ellhip_batch *spaces, ellhip_batch_linfeas *o, int64_t max_iters, double tol,
                                       double *x_out, int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);
int ellhip_batch_linfeas_feas_streamed_stable(ellhip_batch *spaces, ellhip_batch_linfeas *o, int64_t max_iters, double tol,
                                              double *x_out, int32_t *feasible_out, int64_t *niter_out,
                                              int32_t *status_out);

/* ellhip_batch_linfeas_bsearch on a streamed handle: same arguments, semantics, outputs and refusals, with the handle's
 * kind as above.  Afterwards the handle's matrix, kappa and tsq are untouched in every bit and its xc is the x of the last
 * feasible probe. */
int ellhip_batch_linfeas_bsearch_streamed(ellhip_batch *spaces, ellhip_batch_linfeas *o, const double *lower,
                                          const double *upper, int64_t inner_max_iters, double inner_tol, int64_t max_iters,
                                          double tol, int32_t *feasible_out, int64_t *niter_out, double *upper_out,
                                          int64_t *rounds_out, int64_t *ends_out);
int ellhip_batch_linfeas_bsearch_streamed_stable(ellhip_batch *spaces, ellhip_batch_linfeas *o, const double *lower,
                                                 const double *upper, int64_t inner_max_iters, double inner_tol,
                                                 int64_t max_iters, double tol, int32_t *feasible_out, int64_t *niter_out,
                                                 double *upper_out, int64_t *rounds_out, int64_t *ends_out);

#ifdef __cplusplus
}
#endif
#endif
