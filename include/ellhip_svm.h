/*
 * ellhip_svm.h -- C ABI of the device-side SvmOracle and of the device-resident cutting-plane loop
 * built on it (libellhip.so).
 *
 * Reference: `SvmOracle` (src/oracles/svm_oracle.rs:4-58): an m x nfeat table of samples, their
 * i32 labels, and per call the margin y_i * (w.x_i + b) of every sample with w = x[0..nfeat),
 * b = x[nfeat]; the cut comes from the sample with the smallest margin.  The search space has
 * dimension n = nfeat + 1.  A Rust binding keeps the table on the device behind this handle and
 * implements `OracleOptim<Arr>` (src/cutting_plane.rs:129-136) by calling ellhip_svm_assess_optim
 * (see INTEGRATION.md section 11).
 *
 * Every value is the reference's to the bit: each margin is the reference's left fold of the
 * products (starting from -0.0, as current Rust's `Sum for f64` does; this only decides the sign of
 * a margin that is an exact zero), and the argmin keeps the reference's rule (first index among
 * equal minima, NaN and +inf never win).
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, plain pointers and sizes, 0 = ok,
 * negative = ELLHIP_E_*, no CPU fallback.
 */
#ifndef ELLHIP_SVM_H
#define ELLHIP_SVM_H

#include "ellhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellhip_svm ellhip_svm;

/* SvmOracle::new(data, labels) (:11-19).  `data`: m x nfeat, row-major; `labels`: m values.  The table is
 * stored on the device feature-major (m * nfeat * 8 bytes plus padding), transposed there from bounded
 * slabs of the caller's table.  m >= 1 and nfeat >= 1, else ELLHIP_E_INVALID; ELLHIP_E_NODEVICE without a
 * HIP device. */
int ellhip_svm_create(ellhip_svm **out, int64_t m, int64_t nfeat, const double *data, const int32_t *labels,
                      int device);
void ellhip_svm_destroy(ellhip_svm *o);

/* OracleOptim::assess_optim(&mut self, xc, &mut gamma) -> ((Arr, SingleCut), bool) (:24-58).
 * x[nfeat + 1]; grad_out[nfeat + 1]; *beta_out is the SingleCut's value; *shrunk_out is always 1.  The
 * incoming *gamma_inout is ignored; it receives min_val, or +0.0 when min_val >= 1.0 (then the gradient
 * is the zero vector and beta is 0.0).  Returns 1 (a cut is always produced). */
int ellhip_svm_assess_optim(ellhip_svm *o, const double *x, double *gamma_inout, double *grad_out, double *beta_out,
                            int *shrunk_out);

/* All m margins y_i * (w.x_i + b) at x (observability and tests); also sets what ellhip_svm_last reports. */
int ellhip_svm_margins(ellhip_svm *o, const double *x, double *margins_out);

/* The argmin of the last scan (ellhip_svm_assess_optim, ellhip_svm_margins or the last iteration of
 * ellhip_svm_optim): min_idx and min_val as the reference leaves them (0 and +inf when no margin is below
 * +inf). */
int ellhip_svm_last(ellhip_svm *o, int64_t *min_idx, double *min_val);

/* cutting_plane_optim(&mut omega, &mut space, &mut gamma, &Options{max_iters, tolerance})
 * (src/cutting_plane.rs:286-313) with omega = this oracle and space = an UNSHARDED ellhip_space (Ell at
 * any defer depth, or EllStable) of dimension nfeat + 1 on the oracle's device, run entirely on the device
 * (same loop as ellhip_lowpass_optim).  Outputs: x_best_out[nfeat + 1] (written when *has_best_out),
 * *niter_out, *gamma_inout: exactly the reference's (x_best, niter) and gamma.  The space is left in the
 * state the reference loop leaves it in. */
int ellhip_svm_optim(ellhip_space *s, ellhip_svm *o, double *gamma_inout, int64_t max_iters, double tol,
                     double *x_best_out, int *has_best_out, int64_t *niter_out);

#ifdef __cplusplus
}
#endif
#endif
