/*
 * ellhip_batch_bsearch.h -- C ABI of the batched linear feasibility oracles with a movable target and of the batched,
 * device-resident bsearch over them (libellhip.so).
 *
 * The oracle (ellhip_batch_linfeas) is MyOracle3 (src/example3.rs:6-60), the reference's only OracleFeas that implements
 * update(gamma), as a family.  Problem b has J rows A[j][0..n) and offsets c[j], a cursor idx (-1 at first, :15) and a target
 * (-1e100 at first, :16).  assess_feas(x) walks at most J rows cyclically after the cursor (idx += 1; if idx == J { idx = 0 },
 * :29-33); for each it takes
 *
 *     f = 0.0;  for k ascending: f += A[j][k] * x[k]      (two roundings per term, nothing contracted)
 *     fj = f - c[j]  for j < J - 1,   fj = f - target  for j = J - 1     (the last row has no offset: c[J - 1] is never read)
 *
 * and answers the first fj > 0.0 with (A[j], SingleCut(fj)) (:41-52), or None (:54).  update(gamma) sets the target (:57-59).
 * With A = [[-1, 0], [0, -1], [1, 1], [2, -3]] and c = (1, 2, 1, .) this is MyOracle3.  For finite x the folds and the
 * reference's four expressions (:35-38) differ in nothing but the sign of a zero fold; rows 0 to 2 subtract a non-zero offset,
 * which forgets it, and row 3's fj can carry it only where 2 x - 3 y and the target are both zero, where fj is a zero, not
 * > 0.0 and so never handed out: which row answers, and its fj, have the same bits for every finite x and every target
 * (csrc/batch_linfeas_kernels.hpp has the argument line by line).  For a non-finite x the fold is the definition.
 * Limits: n in 1..128, J in 1..512, B <= 2^24.
 *
 * Work split: thread t of a problem (it has n) folds rows t, t + n, ...; the problem's first thread then walks the cursor
 * over the J values.  All J rows are evaluated in every call whether or not the walk reaches them: J n multiply-adds per
 * call against the update's about 2 n^2, and J n doubles read (from L2 when the table is shared).
 *
 * The driver.  ellhip_batch_linfeas_bsearch / _bsearch_stable run, per problem, bsearch (src/cutting_plane.rs:441-466) with
 * BSearchAdaptor::assess_bs (:403-419) as its oracle, in one kernel per chunk of rounds with no host in the loop:
 *
 *     tau = (upper - lower) / 2.0; tau < tol stops with (upper != u_orig, niter)                       :452-455
 *     gamma = lower; gamma += tau                                                                      :456-457
 *     the probe: clone the space, update(gamma), cutting_plane_feas on the clone (:205-227)            :410-412
 *     Some(x): space.set_xc(x), upper = gamma; None: lower = gamma                                     :413-417, :458-463
 *     after max_iters probes (upper != u_orig, max_iters)                                              :465
 *
 * assess_bs never changes the adaptor space's matrix, kappa or tsq, only its centre.  So the batch handle is read-only
 * apart from xc, and a clone is one read of the problem's n^2 doubles from HBM into the LDS block of the workgroup that
 * owns it (8 n^2 bytes per probe and problem); it honours the handle's no_defer_trick, as Clone does.  A probe ends one of
 * four ways, counted in ends_out: [0] a feasible centre (round 0, where no cut is applied at all, included), [1] a cut
 * status other than Success, [2] tsq < inner_tol after a successful cut, [3] inner_max_iters.  The cursor and the target
 * persist across probes and across calls, as self.omega does.
 *
 * A launch runs at most `chunk` rounds (a round is one oracle call), so a launch boundary can fall inside a probe: the
 * probe's matrix, xc, kappa and tsq then wait in buffers of the oracle handle (allocated by the first bsearch call,
 * 8 (n^2 + n + 2) bytes per problem) and the bisection state (120 bytes per problem) beside the cursor.  The host launches
 * at most ceil(max_iters (inner_max_iters + 1) / chunk) times and stops early on the "all stopped" count.
 *
 * The kernel, k_batch_bsearch, is a sibling of the loop kernel of the other batched solves: it shares the oracle policy,
 * the cut (the code ellhip_batch_update runs) and the LDS layout with it, and every earlier kernel compiles to the same
 * instructions as before (profiles/batch_bsearch/resources.txt, which also has the new kernels' registers).
 *
 * Not built: the streamed engines (a streamed handle is refused with a text that says so); update(gamma) hooks for the LMI,
 * low-pass and SVM oracles, whose OracleFeas::update in the reference is the trait's no-op (src/cutting_plane.rs:125).
 *
 * Measured: not measured.  tools/batch_bsearch_bench.py times the device driver against the host-driven form (bisection in
 * numpy, each probe a fresh batch handle, set_target, feas, set_xc) and one CPU thread, and refuses to print a rate unless
 * the three agree in every bit; no run of it could be made for this text, so there is no rate to quote and no claim that
 * the device driver is ahead at any shape.  Computed, not measured: the clones of a call move 8 n^2 bytes per probe and
 * problem, 1,056 bytes per problem at n = 2 and 67,584 at n = 16 for the 33 probes of the tests' family.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_BSEARCH_H
#define ELLHIP_BATCH_BSEARCH_H

#include "ellhip_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellhip_batch_linfeas ellhip_batch_linfeas;

/* B oracles of J rows in n variables.  shared != 0: a[J][n] and c[J] serve every problem; shared == 0: a[B][J][n], c[B][J].
 * c has J entries per table and the last is never read.  ELLHIP_E_INVALID for B < 1 or B > 2^24, n outside 1..128, J outside
 * 1..512 or a NULL array; these are checked before the device is looked for.  *out is NULL after every failure. */
int ellhip_batch_linfeas_create(ellhip_batch_linfeas **out, int64_t B, int64_t n, int64_t J, const double *a,
                                const double *c, int32_t shared, int device);
void ellhip_batch_linfeas_destroy(ellhip_batch_linfeas *o);
/* rounds per launch (default 256, 1..4096): the host looks at the "all stopped" count between launches */
int ellhip_batch_linfeas_set_chunk(ellhip_batch_linfeas *o, int64_t iters);

/* update(gamma[b]) for every problem (src/example3.rs:57-59) */
int ellhip_batch_linfeas_set_target(ellhip_batch_linfeas *o, const double *gamma);
/* the cursors and the targets as they are: idx_out[B], target_out[B] */
int ellhip_batch_linfeas_state(ellhip_batch_linfeas *o, int32_t *idx_out, double *target_out);

/* assess_feas for every problem at x[B][n]: cut_out[b] = the row that answered, or -1 for None; grad_out[B][n] = that row
 * (zeros for None), beta_out[B] = its fj (0.0 for None).  The cursors advance, as the reference's do. */
int ellhip_batch_linfeas_assess_feas(ellhip_batch_linfeas *o, const double *x, double *grad_out, double *beta_out,
                                     int32_t *cut_out);

/* cutting_plane_feas (src/cutting_plane.rs:205-227) for every problem on `spaces`, an Ell (feas) or EllStable (feas_stable)
 * batch handle of the LDS engine with the same B, n and device, which it changes as the reference's loop changes its space.
 * x_out[B][n] (rows with feasible_out[b] == 0 untouched; may be NULL); niter_out[B]; status_out[B] as ellhip_batch_lmi_feas.
 * Refusals (ELLHIP_E_INVALID, nothing touched) as for bsearch below. */
int ellhip_batch_linfeas_feas(ellhip_batch *spaces, ellhip_batch_linfeas *o, int64_t max_iters, double tol, double *x_out,
                              int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);
int ellhip_batch_linfeas_feas_stable(ellhip_batch *spaces, ellhip_batch_linfeas *o, int64_t max_iters, double tol,
                                     double *x_out, int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);

/* bsearch over BSearchAdaptor for every problem, on the device.  spaces: the adaptor's `space`, an Ell (bsearch) or EllStable
 * (bsearch_stable) batch handle of the LDS engine with the same B, n and device; afterwards its matrix, kappa and tsq are
 * untouched in every bit (an EllStable handle's scratch triangle included) and its xc is the x of the last feasible probe.
 * lower[B], upper[B]: the interval (:447); (inner_max_iters, inner_tol): the adaptor's options; (max_iters, tol): bsearch's.
 * feasible_out[B] and niter_out[B] are the reference's (bool, usize).  upper_out[B] (the final upper bound; the reference
 * does not write intrvl back), rounds_out[B] (oracle calls, summed over the probes) and ends_out[B][4] (how the probes
 * ended, see above; may be NULL) are additions.  Refused with ELLHIP_E_INVALID, spaces, oracle and outputs untouched: a
 * streamed handle, a handle of the other variant, a B, n or device mismatch, negative iteration counts, and lower[b] >
 * upper[b] (or a NaN bound) for any b, where the reference asserts (:448). */
int ellhip_batch_linfeas_bsearch(ellhip_batch *spaces, ellhip_batch_linfeas *o, const double *lower, const double *upper,
                                 int64_t inner_max_iters, double inner_tol, int64_t max_iters, double tol,
                                 int32_t *feasible_out, int64_t *niter_out, double *upper_out, int64_t *rounds_out,
                                 int64_t *ends_out);
int ellhip_batch_linfeas_bsearch_stable(ellhip_batch *spaces, ellhip_batch_linfeas *o, const double *lower,
                                        const double *upper, int64_t inner_max_iters, double inner_tol, int64_t max_iters,
                                        double tol, int32_t *feasible_out, int64_t *niter_out, double *upper_out,
                                        int64_t *rounds_out, int64_t *ends_out);

#ifdef __cplusplus
}
#endif
#endif
