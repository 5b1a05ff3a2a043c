/*
 * ellhip_batch_svm.h -- C ABI of the batched, device-resident cutting-plane loop for SVM problems (libellhip.so;
 * DESIGN.md section 9.4).
 *
 * B independent `SvmOracle`s (src/oracles/svm_oracle.rs:4-58) of one shape: m samples of nfeat features each, either one
 * table shared by every problem (one-vs-rest over one table, label-noise sweeps) or one table per problem
 * (cross-validation folds, bootstrap replicas), and m labels per problem.  The search space has n = nfeat + 1 <= 128
 * dimensions: w = x[0..nfeat), b = x[nfeat].  One `assess_optim` (:27-57) takes margin_i = labels[i] as f64 *
 * (dot(w, data[i]) + b) for every sample, the dot product folded left to right from -0.0 (Arr::dot, src/arr.rs:443-451),
 * and the argmin under the reference's scan (:31-40): min_val starts at +inf and min_idx at 0, only `margin < min_val`
 * replaces the minimum, so the first of equal margins wins (-0.0 == +0.0) with its own bits and NaN or +inf never win.
 * min_val >= 1.0 answers the zero cut (n zeros, beta 0.0, gamma +0.0; :42-45), otherwise g = -y [data[min_idx], 1],
 * beta = gamma = min_val (:47-57).  `shrunk` is always true.
 *
 * ellhip_batch_svm_optim runs `cutting_plane_optim` (src/cutting_plane.rs:286-313) for every problem on the device: one
 * workgroup-resident ellipsoid per problem (an ellhip_batch handle of `Ell` spaces), oracle and update in the same kernel,
 * no host in the loop.  Margins, chosen samples, cuts, iteration counts, x_best, gamma, the oracle state and the spaces
 * afterwards are bit-identical to the CPU arithmetic.  (ellhip_svm.h serves one problem with millions of samples; this
 * one sweeps of small problems.)  SvmOracle implements OracleOptim only, so there is no `_feas` entry point.
 *
 * `EllStable` batch handles belong to ellhip_batch_stable_loops.h (ellhip_batch_svm_optim_stable): ellhip_batch_svm_optim
 * refuses them with ELLHIP_E_INVALID.  Problems of up to 1023 features and streamed batch handles belong to
 * ellhip_batch_svm_streamed.h; the entry points of this header keep refusing both.
 *
 * Memory: the table is kept feature-major on the device, nfeat x ld doubles per table with ld = m rounded up to 8; it is
 * transposed on the device at create from bounded slabs of the caller's rows.
 *
 * LDS: a workgroup holds `epw` problems, epw as the batch engine chooses it for n (ellhip_batch.h).  With p(k) = k | 1
 * it needs
 *
 *     epw * 8 * ( ((n * p(n) + 2 n + 8) | 1)  +  ((n + 10) | 1) )   bytes,
 *
 * the first term being the batch engine's own (matrix, gradient, Q g, scalars), the second the oracle's (x, the loop's
 * scalars and the two words of the argmin merge); the table stays in HBM / L2.  A shape that needs more than 159 KiB (the
 * device's 160 KiB per workgroup less 1 KiB the kernel keeps for itself) is refused by ellhip_batch_svm_optim; every
 * n <= 128 fits (n = 128: 131.1 KiB + 1.1 KiB = 132.2 KiB).
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_SVM_H
#define ELLHIP_BATCH_SVM_H

#include "ellhip_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellhip_batch_svm ellhip_batch_svm;

/* SvmOracle::new(data[b], labels[b]) for b = 0..B-1 (:15-17).  shared_data != 0: `data` is one row-major m x nfeat table
 * used by every problem; shared_data == 0: `data` is [B][m][nfeat].  labels: [B][m] int32 in both cases, any value
 * (`labels[i] as f64` is the multiplier, :32).  ELLHIP_E_INVALID for B <= 0 or B > 2^24, m < 1 or m > 2^24, nfeat < 1 or
 * nfeat > 127 (n = nfeat + 1 <= ELLHIP_BATCH_NMAX), NULL data or labels; these are checked before the device. */
int ellhip_batch_svm_create(ellhip_batch_svm **out, int64_t B, int64_t m, int64_t nfeat, const double *data,
                            int32_t shared_data, const int32_t *labels, int device);
void ellhip_batch_svm_destroy(ellhip_batch_svm *o);

/* All margins of every problem at x[B][n] into margins_out[B][m] (observability and tests; the state that
 * ellhip_batch_svm_last reports is not touched). */
int ellhip_batch_svm_margins(ellhip_batch_svm *o, const double *x, double *margins_out);
/* assess_optim (:27-57) for every problem at x[B][n]: gamma_out[B], grad_out[B][n], beta_out[B].  `shrunk` is always true
 * and the incoming gamma is ignored, as ellhip_svm_assess_optim documents.  Where min_val >= 1.0 the gradient is n zeros
 * (+0.0), beta 0.0 and gamma +0.0. */
int ellhip_batch_svm_assess_optim(ellhip_batch_svm *o, const double *x, double *gamma_out, double *grad_out,
                                  double *beta_out);
/* The argmin of each problem's last scan (assess_optim or the loop): min_idx[B], min_val[B]; 0 and +inf when no margin
 * was below +inf, and after create.  Either may be NULL. */
int ellhip_batch_svm_last(ellhip_batch_svm *o, int64_t *min_idx, double *min_val);

/* cutting_plane_optim (src/cutting_plane.rs:286-313) for every problem, on the device.  spaces: an Ell batch handle with
 * the same B, n = nfeat + 1 and device.  gamma_inout[B]; x_best_out[B][n] (rows with has_best_out[b] == 0 untouched; may
 * be NULL); niter_out[B]; status_out[B] = the CutStatus of the last update (Success when the tolerance or max_iters ended
 * the loop).  Afterwards the spaces and the oracle state (ellhip_batch_svm_last) are exactly what the reference loop
 * leaves (the update that hit the tolerance is complete; after the reference's zero cut the space is NaN), so
 * ellhip_batch_update, the getters and a second call continue from there.  Refused with ELLHIP_E_INVALID, spaces and
 * outputs untouched: an EllStable batch handle, a B, n or device mismatch, a shape beyond the LDS bound above. */
int ellhip_batch_svm_optim(ellhip_batch *spaces, ellhip_batch_svm *o, double *gamma_inout, int64_t max_iters, double tol,
                           double *x_best_out, int32_t *has_best_out, int64_t *niter_out, int32_t *status_out);
/* iterations per launch (default 256, 1..4096): the host looks at the "all stopped" count between launches */
int ellhip_batch_svm_set_chunk(ellhip_batch_svm *o, int64_t iters);

#ifdef __cplusplus
}
#endif
#endif
