/*
 * ellhip_batch_stable_loops.h -- C ABI of the batched, device-resident cutting-plane loops on `EllStable` search spaces
 * (libellhip.so).
 *
 * ellhip_batch_lmi.h, ellhip_batch_lowpass.h and ellhip_batch_svm.h run B small problems, oracle and ellipsoid update in
 * one kernel, on an ellhip_batch handle of `Ell` spaces.  The five entry points below run the same loops over the same
 * oracle handles on a handle of `EllStable` spaces (src/ell_stable.rs; ellhip_batch_create_stable,
 * ellhip_batch_stable_from_space), as the reference drives its LMI problems through both spaces
 * (tests/lmi_tests.rs:201-225).  The oracles, the loop state, the stopping rule (`status != Success || tsq < tol`,
 * src/cutting_plane.rs:222, 308), feasibility stops, the x_best rule, the chunked relaunch (the oracle handle's
 * `_set_chunk`) and every argument are those of the Ell counterpart; only the update differs.
 *
 * The update is `EllStable::update_core` (src/ell_stable.rs:52-125) on the packed buffer in LDS (diagonal = D, strict
 * upper = the factor, strict lower = scratch), spread over the n threads of a problem: the forward solve right-looking
 * with one workgroup barrier per column, omega, `EllCalc` and the `temp` chain of the rank-one update on one lane per
 * problem, the back solve serial on one thread, the factor's columns and the diagonal one thread each.  Nothing is
 * parallelised inside a fold, so iteration counts, x_best, gamma, the oracle state and the spaces afterwards (`mq` with
 * its scratch triangle, `xc`, `kappa`, `tsq`) are bit-identical to the CPU arithmetic and to the host-driven form over
 * ellhip_batch_update.  A failed cut leaves everything but `tsq` and the scratch triangle untouched (:88-90).  Cuts with
 * two values go through `EllStable`'s update_bias_cut (:139-145; src/ell_calc.rs) and honour
 * ellhip_batch_set_use_parallel_cut.
 *
 * LDS: a workgroup of T threads (256 for n <= 64, else 128) holds epw = min(64, T / n) problems, fewer while
 * epw * 8 * s(n) exceeds 64 KiB, with p(k) = k | 1 and
 *
 *     s(n) = (n * p(n) + 3 n + 8) | 1        doubles: the buffer, three n-vectors, 8 scalars.
 *
 * A launch needs epw * 8 * (s(n) + the oracle's term of the Ell counterpart's header) bytes; a shape that needs more than
 * 159 KiB is refused.  n = 128 fits for low-pass and SVM and for LMI blocks of M <= 8, as on Ell.
 *
 * Refused with ELLHIP_E_INVALID, spaces and outputs untouched: an Ell batch handle (as ellhip_batch_stable_from_space
 * refuses an Ell space), a B, n or device mismatch between spaces and oracle, a shape beyond the LDS bound, and whatever
 * the Ell counterpart refuses.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_STABLE_LOOPS_H
#define ELLHIP_BATCH_STABLE_LOOPS_H

#include "ellhip_batch_lmi.h"
#include "ellhip_batch_lowpass.h"
#include "ellhip_batch_svm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cutting_plane_optim (src/cutting_plane.rs:286-313) over the round-robin LMI oracle (tests/lmi_tests.rs:142-171) on
 * EllStable spaces (tests/lmi_tests.rs:201-225); arguments as ellhip_batch_lmi_optim. */
int ellhip_batch_lmi_optim_stable(ellhip_batch *spaces, ellhip_batch_lmi *o, double *gamma_inout, int64_t max_iters,
                                  double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                                  int32_t *status_out);
/* cutting_plane_feas (src/cutting_plane.rs:205-227) with the J blocks as stations; arguments as ellhip_batch_lmi_feas. */
int ellhip_batch_lmi_feas_stable(ellhip_batch *spaces, ellhip_batch_lmi *o, int64_t max_iters, double tol, double *x_out,
                                 int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);

/* cutting_plane_optim over LowpassOracle::assess_optim (src/oracles/lowpass_oracle.rs:139-150); arguments as
 * ellhip_batch_lowpass_optim.  The oracle's parallel cuts are EllStable's update_bias_cut with Some(beta1)
 * (src/ell_stable.rs:139-145). */
int ellhip_batch_lowpass_optim_stable(ellhip_batch *spaces, ellhip_batch_lowpass *o, double *gamma_inout,
                                      int64_t max_iters, double tol, double *x_best_out, int32_t *has_best_out,
                                      int64_t *niter_out, int32_t *status_out);
/* cutting_plane_feas over LowpassOracle::assess_feas (src/oracles/lowpass_oracle.rs:58-135); arguments as
 * ellhip_batch_lowpass_feas. */
int ellhip_batch_lowpass_feas_stable(ellhip_batch *spaces, ellhip_batch_lowpass *o, int64_t max_iters, double tol,
                                     double *x_out, int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);

/* cutting_plane_optim over SvmOracle::assess_optim (src/oracles/svm_oracle.rs:27-57), every cut a central cut
 * (src/ell_stable.rs:147-153); arguments as ellhip_batch_svm_optim. */
int ellhip_batch_svm_optim_stable(ellhip_batch *spaces, ellhip_batch_svm *o, double *gamma_inout, int64_t max_iters,
                                  double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                                  int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif
