/*
 * ellhip_batch_profit.h -- C ABI of the batched, device-resident cutting-plane loops for profit-maximisation problems
 * (libellhip.so), and of the discrete driver cutting_plane_optim_q.
 *
 * B independent problems of two variables y = (ln x1, ln x2): maximise p A x1^a1 x2^a2 - v1 x1 - v2 x2 subject to x1 <= k
 * (src/oracles/profit_oracle.rs), as a sweep over prices, elasticities and robustness margins.  Three kinds of oracle:
 *
 *   ELLHIP_PROFIT_PLAIN     ProfitOracle (:7-79).  A cursor walks the two constraints and persists across calls:
 *                           0: fj = y[0] - ln k, gradient (1, 0);
 *                           1: log_cobb = ln(p A) + (a . y) (the dot product a left fold from +0.0), q = v o exp(y),
 *                              vx = q[0] + q[1], fj = ln(gamma + vx) - log_cobb, gradient q / (gamma + vx) - a.
 *                           The first fj > 0 is the cut (`shrunk` false).  With none: gamma = exp(log_cobb) - vx, gradient
 *                           q / exp(log_cobb) - a, beta = 0, `shrunk` true.
 *   ELLHIP_PROFIT_ROBUST    ProfitRbOracle (:82-126): per call a[i] - uie[i] where y[i] > 0.0 and a[i] + uie[i] elsewhere,
 *                           then the plain oracle built from (p - e3, A, k - e4) and v + e5 (vparams = (uie1, uie2, e3, e4, e5)).
 *   ELLHIP_PROFIT_DISCRETE  ProfitOracleQ (:128-163), an OracleOptimQ.  retry false: a cut of the plain oracle's constraints at y
 *                           is handed out with x_q = y and more_alt true; with none, x_disc = round(exp(y)) (half away from
 *                           zero, zeros replaced by 1) and yd = ln(x_disc).  Then, and on a retry with the yd it kept:
 *                           the plain assess_optim at yd, beta += grad . (yd - y), x_q = yd, more_alt = !retry.
 *
 * Arithmetic.  exp and ln are ell_exp and ell_log (csrc/ell_math.hpp): + - * / and integer operations on the representation
 * only, the same roundings on the host and on the device, at most 0.718 ulp (exp) and 0.772 ulp (log) from the exact value
 * over the test sweep (measured against mpmath; glibc documents 1 ulp for both).  The constructor's ln(p A) and ln(k) go
 * through ell_log too.  Every operation keeps the reference's order and nothing is contracted, so cuts, gamma, iteration
 * counts, x_best and the spaces afterwards are bit-identical to the reference's loops restated with these two functions
 * (tests/batch_profit_reference.py); against the same loops with glibc's exp and log the iteration counts of the reference's
 * three pinned cases (83, 90, 29) are kept and gamma and x_best agree to 1e-6 relative.
 *
 * ellhip_batch_profit_optim / _optim_stable run cutting_plane_optim (src/cutting_plane.rs:286-313) for the plain and the
 * robust kind, ellhip_batch_profit_optim_q / _optim_q_stable run cutting_plane_optim_q (:331-374) for the discrete kind:
 * x_best is the oracle's point x_q, every cut is a discrete one (update_q, ELLHIP_CUT_Q), NoSoln ends the loop, NoEffect ends
 * it unless the oracle has another cut to offer (more_alt), in which case the oracle is asked again with retry = true, the
 * space untouched and the iteration counted.  Oracle, update and driver are one kernel, no host in the loop, on the two LDS
 * engines (ellhip_batch.h: Ell and EllStable batch handles).  n = 2, so there is no streamed form.
 *
 * Work split: a problem has two threads; each takes ell_exp of one coordinate, the first of them does the rest (the
 * constraints, one ell_log, one ell_exp when feasible; in the discrete kind's feasible rounds two more of each).
 *
 * LDS: the oracle adds 25 doubles per problem (the point, its exps, yd, 18 scalars) to the engine's own.  With epw = 64
 * problems per workgroup (ellhip_batch.h) a workgroup needs
 *
 *     optim, optim_q                  epw * 8 * ( ((n (n|1) + 2 n + 8) | 1) + 25 ) = 64 * 8 * (19 + 25) = 22,528 bytes
 *     optim_stable, optim_q_stable    epw * 8 * ( ((n (n|1) + 3 n + 8) | 1) + 25 ) = 64 * 8 * (21 + 25) = 23,552 bytes
 *
 * Registers (gfx950, no scratch in any of them; profiles/batch_profit/resources.txt): k_batch_loop<T, false / true, .> 97 / 107
 * VGPRs for the plain and robust kinds, 93 / 111 for the discrete kind under the optim_q driver; k_batch_profit_assess 40
 * and 50.  The loop kernels that existed before the optim_q driver compile to the same instructions as before.
 *
 * Measured (MI355X, tools/batch_profit_bench.py: the first 64 members of the tests' seeded family repeated to B, whole solves
 * with the reference's default options from new_with_scalar(100, xc0) and gamma = 0; host clock around the whole call, median
 * of 20 calls after 3 warm-up calls; the calls are short -- 0.5 to 0.7 ms up to B = 16384, which is a call's fixed costs, 3
 * to 4 ms at B = 262144 -- and min and max lie within 1 % to 47 % of the median), rounds per second of all problems together
 * -- the device loop, the host-driven form (one wide assess and one ellhip_batch_update per iteration) and a one-thread CPU
 * loop with the same exp and log:
 *
 *     (kind, B)            Ell: loop   host-driven   CPU       EllStable: loop   host-driven   CPU
 *     plain, 1024          1.5e8       2.8e6         1.2e7     1.4e8             2.0e6         1.1e7
 *     plain, 262144        6.0e9       4.1e7         1.2e7     6.4e9             3.9e7         1.1e7
 *     plain, 2097152       4.5e9       3.6e7         1.2e7     4.9e9             3.4e7         1.1e7
 *     robust, 1024         1.5e8       2.7e6         1.2e7     1.5e8             2.9e6         1.1e7
 *     robust, 262144       6.4e9       4.5e7         1.1e7     6.6e9             4.8e7         1.1e7
 *     robust, 2097152      4.9e9       4.4e7         1.2e7     5.2e9             4.3e7         1.1e7
 *     discrete, 1024       6.7e7       2.0e6         7.9e6     6.2e7             1.3e6         7.3e6
 *     discrete, 262144     2.4e9       3.3e7         7.9e6     2.6e9             3.3e7         7.3e6
 *     discrete, 2097152    1.8e9       3.1e7         7.9e6     1.7e9             2.6e7         7.3e6
 *
 * The device loop is ahead of the host-driven form at every shape (34 to 164 times).  At B = 2097152 the call is slowed by
 * its own result copies (40 bytes per problem).  DESIGN.md section 9.13 has B = 16384 and the discussion.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_PROFIT_H
#define ELLHIP_BATCH_PROFIT_H

#include "ellhip_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellhip_batch_profit ellhip_batch_profit;

#define ELLHIP_PROFIT_PLAIN 0
#define ELLHIP_PROFIT_ROBUST 1
#define ELLHIP_PROFIT_DISCRETE 2

/* The constructors of the three oracles for b = 0..B-1: params[B][3] = (p, A, k), elasticities[B][2] = a, price_out[B][2] = v,
 * vparams[B][5] for the robust kind and NULL for the others.  ELLHIP_E_INVALID for B < 1 or B > 2^24, an unknown kind, a NULL
 * array, vparams with a kind that takes none or missing for the robust one; these are checked before the device is looked
 * for.  *out is NULL after every failure. */
int ellhip_batch_profit_create(ellhip_batch_profit **out, int64_t B, int32_t kind, const double *params,
                               const double *elasticities, const double *price_out, const double *vparams, int device);
void ellhip_batch_profit_destroy(ellhip_batch_profit *o);
/* iterations per launch (default 256, 1..4096): the host looks at the "all stopped" count between launches */
int ellhip_batch_profit_set_chunk(ellhip_batch_profit *o, int64_t iters);

/* assess_optim for every problem at x[B][2] (plain and robust kinds): gamma_inout[B] is read and, where `shrunk`, replaced;
 * grad_out[B][2]; beta_out[B]; shrunk_out[B].  The last two may be NULL.  The cursors advance, as the reference's do. */
int ellhip_batch_profit_assess_optim(ellhip_batch_profit *o, const double *x, double *gamma_inout, double *grad_out,
                                     double *beta_out, int32_t *shrunk_out);
/* assess_optim_q for every problem (discrete kind) with retry[B]; also x_q_out[B][2] and more_alt_out[B] (may be NULL).  The
 * cursors advance and yd is kept for a later retry. */
int ellhip_batch_profit_assess_optim_q(ellhip_batch_profit *o, const double *x, double *gamma_inout, const int32_t *retry,
                                       double *grad_out, double *beta_out, int32_t *shrunk_out, double *x_q_out,
                                       int32_t *more_alt_out);

/* cutting_plane_optim (optim, optim_stable: plain and robust kinds) or cutting_plane_optim_q (optim_q, optim_q_stable:
 * discrete kind) for every problem, on the device.  spaces: an Ell (optim, optim_q) or EllStable (_stable) batch handle of the
 * LDS engine with n = 2 and the same B and device.  gamma_inout[B]; x_best_out[B][2] (rows with has_best_out[b] == 0
 * untouched; may be NULL); niter_out[B]; status_out[B] = the CutStatus that ended the loop (Success when the tolerance or
 * max_iters ended it).  Afterwards the spaces are exactly what the reference loop leaves, and the cursors and yd are kept, so
 * ellhip_batch_update, the getters and a second call continue from there; every call starts with retry = false, as the
 * reference's does.  Refused with ELLHIP_E_INVALID, spaces and outputs untouched: a handle with n != 2, a B or device
 * mismatch, a handle of the other variant, a streamed handle, a kind that belongs to the other pair of entry points. */
int ellhip_batch_profit_optim(ellhip_batch *spaces, ellhip_batch_profit *o, double *gamma_inout, int64_t max_iters,
                              double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                              int32_t *status_out);
int ellhip_batch_profit_optim_stable(ellhip_batch *spaces, ellhip_batch_profit *o, double *gamma_inout, int64_t max_iters,
                                     double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                                     int32_t *status_out);
int ellhip_batch_profit_optim_q(ellhip_batch *spaces, ellhip_batch_profit *o, double *gamma_inout, int64_t max_iters,
                                double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                                int32_t *status_out);
int ellhip_batch_profit_optim_q_stable(ellhip_batch *spaces, ellhip_batch_profit *o, double *gamma_inout, int64_t max_iters,
                                       double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                                       int32_t *status_out);

/* Test support in the ABI, as ellhip_calc: out[j] = ell_exp(x[j]) (fn = 0) or ell_log(x[j]) (fn = 1) for j < count, on the
 * device. */
int ellhip_math_eval(int32_t fn, int64_t count, const double *x, double *out, int device);

#ifdef __cplusplus
}
#endif
#endif
