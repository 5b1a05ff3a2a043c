/*
 * ellhip_batch_maxcut.h -- C ABI of the batched, device-resident cutting-plane loops for max-cut problems (libellhip.so;
 * DESIGN.md section 9.12).
 *
 * B independent `MaxcutOracle`s (src/oracles/maxcut_oracle.rs:4-50) of one size n <= 1024: one graph from many starting
 * centres (one weight table shared by every problem) or many graphs of one size (one table per problem).  `weights` is a
 * row-major n x n table of any values; it need not be symmetric.  One `assess_optim` (:21-49) at the centre xc takes
 *
 *   signs      x[i] = xc[i] >= 0.0 ? 1.0 : -1.0 (:22), so -0.0 gives +1 and NaN gives -1;
 *   cut_value  from +0.0, for i ascending and j = i+1 .. n-1 ascending, cut_value += w[i][j] where x[i] != x[j] (:24-31):
 *              one left fold over the upper triangle in row-major order, never re-associated;
 *   gradient   grad[i] from +0.0, for j = 0 .. n-1 ascending, grad[i] += w[i][j] where x[i] != x[j] (:33-40): full rows,
 *              so a table that is not symmetric shows, and the diagonal never contributes; then grad[i] *= 2.0 (:41) and
 *              the gradient handed out is -grad[i], so a zero sum is handed out as -0.0;
 *   improved   cut_value > gamma (strict, NaN is false; :43): gamma = cut_value, the cut is (-grad, -cut_value) and
 *              `shrunk` is true -- the loop keeps the centre as x_best and takes a central cut (src/cutting_plane.rs:301-304;
 *              the beta is carried and ignored);
 *   otherwise  the cut is (-grad, gamma) and `shrunk` is false (:47): a deep cut with beta = gamma (:306).
 *
 * The oracle keeps no state between calls other than gamma.  The only arithmetic is `+`, `* 2.0`, negation and comparisons,
 * and both folds keep the reference's order (a skipped term is added as +0.0, which changes no bit of a fold that starts at
 * +0.0), so cut values, gradients, cuts, iteration counts, x_best, gamma and the spaces afterwards are bit-identical to the
 * CPU arithmetic.  MaxcutOracle implements OracleOptim only, so there is no `_feas` entry point.
 *
 * ellhip_batch_maxcut_optim and its three siblings run `cutting_plane_optim` (src/cutting_plane.rs:286-313) for every
 * problem on the device, oracle and update in one kernel, no host in the loop, on each of the four batch engines:
 *
 *   ellhip_batch_maxcut_optim                  Ell batch handle (ellhip_batch.h), n <= 128, matrices in LDS
 *   ellhip_batch_maxcut_optim_stable           EllStable batch handle, n <= 128
 *   ellhip_batch_maxcut_optim_streamed         streamed Ell batch handle (ellhip_batch_streamed.h), n <= 1024
 *   ellhip_batch_maxcut_optim_streamed_stable  streamed EllStable batch handle (ellhip_batch_streamed_stable.h), n <= 1024
 *
 * Memory: the table is kept row-major on the device as given (the cut value's fold reads it) and a second time transposed
 * (the gradient's fold: at column j the n threads of a problem read n consecutive doubles), 2 * 8 n^2 bytes per table; the
 * transpose is made on the device at create from bounded slabs of whole tables.  When every table is symmetric to the bit
 * the handle keeps the row-major copy alone, 8 n^2 bytes per table.
 *
 * The chain.  cut_value is n (n-1) / 2 dependent adds by one lane (523,776 at n = 1024) and sets the pace of a round, as
 * EllStable's back solve does; the other threads stage its terms through LDS n at a time, masked, in ceil((n-1) / 2) steps
 * of one barrier each, and run their own gradient folds meanwhile, so the lane never waits on global memory.
 *
 * LDS: the oracle adds ((3 n + 8) | 1) doubles per problem (the signs, a double buffer of n terms and the scalars) to the
 * engine's own.  With p(k) = k | 1, e(k) = k rounded up to even and epw the problems per workgroup (ellhip_batch.h) a
 * workgroup needs
 *
 *     optim                    epw * 8 * ( ((n p(n) + 2 n + 8) | 1) + ((3 n + 8) | 1) )   bytes   n = 128: 134.1 KiB
 *     optim_stable             epw * 8 * ( ((n p(n) + 3 n + 8) | 1) + ((3 n + 8) | 1) )           n = 128: 135.1 KiB
 *     optim_streamed           8 * ( 5 e(n) + 8  + ((3 n + 8) | 1) )                              n = 1024: 64.1 KiB
 *     optim_streamed_stable    8 * ( 4 e(n) + 72 + ((3 n + 8) | 1) )                              n = 1024: 56.6 KiB
 *
 * A shape that needs more than 159 KiB (the device's 160 KiB per workgroup less 1 KiB the kernel keeps for itself) is
 * refused; every shape the engines take fits.
 *
 * Traffic per round and problem: the upper triangle once for the chain (4 n^2 bytes) and the transposed table once for the
 * gradient (8 n^2 bytes), the order of the update's own 16 n^2 (streamed Ell) or 24 n^2 (streamed EllStable) bytes; a shared
 * table is served from the caches.
 *
 * Registers (gfx950, no scratch in any of them): k_batch_loop<T, false, .> 132 VGPRs, k_batch_loop<T, true, .> 138 (blocks of
 * at most 256 threads); k_batch_streamed_loop 121 and k_batch_streamed_loop_stable 114, bounded for 1024 threads (128 VGPRs a
 * wave); k_batch_maxcut_assess 88 in its three shapes.  The chain lane keeps two groups of eight values in flight; a third
 * group does not fit under the 128-VGPR bound of the streamed loops.
 *
 * Measured (MI355X, tools/batch_maxcut_bench.py: one shared "mixed" table, 16 starting centres repeated to B, a fixed round
 * count per shape, median of 5 whole calls after 2 warm-up calls, min and max within 2 % of the median), rounds per second of
 * all problems together -- the device loop, the host-driven form (one wide ellhip_batch_maxcut_assess_optim and one
 * ellhip_batch_update per iteration) and a one-thread CPU loop -- and the oracle's share of a round (1 - loop rate / the
 * engine's plain K = 8 update rate):
 *
 *     (n, B)            Ell: loop   host-driven   CPU     share     EllStable: loop   host-driven   CPU     share
 *     (16, 16384)       6.1e8       2.0e7         1.4e6   0.78      3.7e8             1.8e7         1.4e6   0.03
 *     (128, 2048)       2.5e6       1.4e6         3.1e4   0.83      9.5e5             3.3e5         3.0e4   (*)
 *     (129, 1536)       5.5e6       2.2e6         5.2e4   0.76      2.9e6             1.6e6         3.4e4   0.45
 *     (256, 1536)       1.7e6       7.6e5         4.1e3   0.65      9.2e5             5.8e5         6.1e3   0.41
 *     (512, 768)        2.7e5       1.9e5         1.1e3   0.76      1.4e5             1.2e5         1.1e3   0.45
 *     (1024, 256)       4.9e4       4.1e4         2.5e2   0.82      2.6e4             2.4e4         2.6e2   0.45
 *
 * (*) the LDS engine's plain EllStable update runs one lane per ellipsoid and is slower at n = 128 (4.4e5) than the loop,
 * which gives a problem n threads.  The device loop is ahead of the host-driven form at every shape, by 30 times where a
 * round is short and by 1.2 (Ell) and 1.07 (EllStable) at n = 1024, where a round is the chain: 523,776 dependent adds at
 * about 8 ns each, which both forms pay alike.  At n = 128 a workgroup's 134 KiB of LDS leave one problem per compute unit,
 * so the chains of a batch run one after the other; that is the likely reason why the streamed engine, which has several
 * problems on a compute unit, is twice as fast at n = 129.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_MAXCUT_H
#define ELLHIP_BATCH_MAXCUT_H

#include "ellhip_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellhip_batch_maxcut ellhip_batch_maxcut;

/* MaxcutOracle::new(weights[b]) for b = 0..B-1 (:10-15).  shared_weights != 0: `weights` is one row-major n x n table used
 * by every problem; shared_weights == 0: `weights` is [B][n][n].  ELLHIP_E_INVALID for B < 1 or B > 2^24, n < 1 or
 * n > 1024 (ELLHIP_BATCH_STREAMED_NMAX), NULL weights; these are checked before the device is looked for.  *out is NULL
 * after every failure. */
int ellhip_batch_maxcut_create(ellhip_batch_maxcut **out, int64_t B, int64_t n, const double *weights,
                               int32_t shared_weights, int device);
void ellhip_batch_maxcut_destroy(ellhip_batch_maxcut *o);
/* iterations per launch (default 256, 1..4096): the host looks at the "all stopped" count between launches */
int ellhip_batch_maxcut_set_chunk(ellhip_batch_maxcut *o, int64_t iters);

/* assess_optim (:21-49) for every problem at x[B][n], at every n: gamma_inout[B] is read and, where the cut value is
 * larger, replaced; grad_out[B][n] is the gradient handed out (-grad); beta_out[B] is -cut_value where improved, gamma
 * otherwise; shrunk_out[B] is 1 where improved; cut_value_out[B].  The last three may be NULL. */
int ellhip_batch_maxcut_assess_optim(ellhip_batch_maxcut *o, const double *x, double *gamma_inout, double *grad_out,
                                     double *beta_out, int32_t *shrunk_out, double *cut_value_out);

/* cutting_plane_optim (src/cutting_plane.rs:286-313) for every problem, on the device.  spaces: a batch handle of the entry
 * point's engine with the same B, n and device.  gamma_inout[B]; x_best_out[B][n] (the centre itself, not the sign vector;
 * rows with has_best_out[b] == 0 untouched; may be NULL); niter_out[B]; status_out[B] = the CutStatus of the last update
 * (Success when the tolerance or max_iters ended the loop).  Afterwards the spaces are exactly what the reference loop
 * leaves (the update that hit the tolerance is complete), so ellhip_batch_update, the getters and a second call continue
 * from there.  Refused with ELLHIP_E_INVALID, spaces and outputs untouched: a batch handle of another kind than the entry
 * point's, a B, n or device mismatch (an oracle of n > 128 has no LDS-engine handle to match), a shape beyond the LDS bound
 * above. */
int ellhip_batch_maxcut_optim(ellhip_batch *spaces, ellhip_batch_maxcut *o, double *gamma_inout, int64_t max_iters,
                              double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                              int32_t *status_out);
int ellhip_batch_maxcut_optim_stable(ellhip_batch *spaces, ellhip_batch_maxcut *o, double *gamma_inout, int64_t max_iters,
                                     double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                                     int32_t *status_out);
int ellhip_batch_maxcut_optim_streamed(ellhip_batch *spaces, ellhip_batch_maxcut *o, double *gamma_inout,
                                       int64_t max_iters, double tol, double *x_best_out, int32_t *has_best_out,
                                       int64_t *niter_out, int32_t *status_out);
int ellhip_batch_maxcut_optim_streamed_stable(ellhip_batch *spaces, ellhip_batch_maxcut *o, double *gamma_inout,
                                              int64_t max_iters, double tol, double *x_best_out, int32_t *has_best_out,
                                              int64_t *niter_out, int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif
