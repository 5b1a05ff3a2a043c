/*
 * ellhip_batch_svm_streamed.h -- C ABI of the batched, device-resident SVM cutting-plane loop on streamed batch handles
 * (libellhip.so).
 *
 * ellhip_batch_svm.h solves B independent `SvmOracle` problems (src/oracles/svm_oracle.rs:4-58) of one shape (m samples,
 * nfeat features) on the batch engine that keeps each matrix in LDS, so it stops at nfeat = 127 (n = nfeat + 1 <= 128);
 * ellhip_batch_stable_loops.h does the same on EllStable spaces.  This header carries both solves to nfeat <= 1023: the
 * spaces are a streamed batch handle (ellhip_batch_streamed.h for Ell, ellhip_batch_streamed_stable.h for EllStable: the
 * matrices stay in HBM, one workgroup per ellipsoid, one thread per row) and one kernel per chunk of iterations runs
 * `cutting_plane_optim` (src/cutting_plane.rs:286-313) for every problem -- oracle (`assess_optim`, svm_oracle.rs:27-57),
 * x_best, the update (src/ell.rs:96-128 or EllStable::update_core, src/ell_stable.rs:52-125) and the stop test -- with no
 * host in the loop.  The oracle is the device function ellhip_batch_svm.h runs: per-sample fold from -0.0 in ascending
 * feature order, strict-`<` scan, first of equal margins wins with its own bits.  Margins, chosen samples, cuts, iteration
 * counts, x_best, gamma, the oracle state and the spaces afterwards (the NaN space after the zero cut and EllStable's scratch
 * triangle included) are bit-identical to the CPU arithmetic and, at n <= 128, to ellhip_batch_svm_optim / _optim_stable on
 * an LDS handle.
 *
 * The oracle handle is an ordinary ellhip_batch_svm: _destroy, _margins, _assess_optim, _last and _set_chunk of
 * ellhip_batch_svm.h work on it at every n (past n = 128 _margins and _assess_optim run one workgroup of n threads, rounded
 * up to whole waves, per problem).
 *
 * Memory: the table is kept feature-major as ellhip_batch_svm.h describes it, 8 * nfeat * ld bytes per table with ld = m
 * rounded up to 8; one table when shared, B otherwise.  At nfeat = 1023 and m = 8192 that is 64 MiB per table.
 *
 * Traffic per problem and iteration: 16 n^2 bytes of matrix on Ell (`shrunk` is always true and every round but the zero
 * cut's has a gradient, so the product of iteration k + 1 always rides on the sweep of iteration k; the first iteration of a
 * launch adds 8 n^2) or 24 n^2 on EllStable (nothing is fused: the centre is final only after the back solve), plus for the
 * oracle 8 * nfeat * m bytes of table, 4 m of labels and 8 nfeat for the gradient's row.  The table equals an Ell sweep at
 * m = 2 n.  The fold is a chain of ceil(m / n) * nfeat dependent multiply-add pairs per thread.
 *
 * LDS per workgroup, with e(n) = n rounded up to even:
 *
 *     Ell:        8 * (5 e(n) + 8  + ((n + 10) | 1)) bytes, 48.1 KiB at n = 1024;
 *     EllStable:  8 * (4 e(n) + 72 + ((n + 10) | 1)) bytes, 40.6 KiB at n = 1024;
 *
 * both below the 64 KiB a kernel may use without an opt-in, so no shape is refused for LDS.  Compiled for gfx950 and
 * bounded for 1024 threads the two loop kernels take 92 (Ell) and 102 (EllStable) VGPRs and no scratch.
 *
 * Measured on one MI355X (tools/batch_svm_streamed_bench.py; whole calls, rounds per second of all
 * problems together, one table shared by all problems, m = n / 2 ... 8 n samples): on Ell at (n, B) = (129, 1536)
 * 2.4e7 ... 9.0e6, (256, 1536) 4.9e6 ... 2.5e6, (512, 768) 1.2e6 ... 4.9e5, (1024, 256) 3.0e5 ... 1.3e5, which is 221 ... 1068
 * times the CPU loop on one thread, 10.2 ... 1.62 times the host-driven form (one wide ellhip_batch_svm_assess_optim and one
 * ellhip_batch_update per iteration) and 1.08 ... 0.39 of the engine's own update rate at K = 8 cuts per launch; on
 * EllStable at B = 1536 / 512 / 512 / 512: 5.0e6 ... 3.9e6, 1.2e6 ... 9.9e5, 3.4e5 ... 2.8e5, 4.9e4 ... 3.8e4, which is
 * 99 ... 401 times, 3.06 ... 1.08 times and 1.06 ... 0.74.  The scan's share of a round is about 0.1 at m = n / 2 and 0.5 ... 0.7
 * at m = 8 n on Ell, 0.01 ... 0.03 and 0.2 ... 0.3 on EllStable.  The device loop was faster than the host-driven form at every
 * shape measured; on EllStable at n = 1024, where the serial back solve sets the pace, by 5 ... 24 per cent only.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_SVM_STREAMED_H
#define ELLHIP_BATCH_SVM_STREAMED_H

#include "ellhip_batch_svm.h"
#include "ellhip_batch_streamed.h"
#include "ellhip_batch_streamed_stable.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ellhip_batch_svm_create for 1 <= nfeat <= ELLHIP_BATCH_STREAMED_NMAX - 1 (1023); every other argument and refusal as
 * there, checked before the device. */
int ellhip_batch_svm_create_streamed(ellhip_batch_svm **out, int64_t B, int64_t m, int64_t nfeat, const double *data,
                                     int32_t shared_data, const int32_t *labels, int device);

/* ellhip_batch_svm_optim on a streamed handle: same arguments, semantics and outputs.  spaces must be a streamed batch
 * handle (ellhip_batch_is_streamed) of Ell spaces with the oracle's B, n = nfeat + 1 and device; a streamed handle of
 * n <= 128 is accepted.  Anything else -- an LDS handle, a streamed EllStable handle, a mismatch, a NULL argument -- is
 * ELLHIP_E_INVALID with a message, and the spaces and outputs are left untouched. */
int ellhip_batch_svm_optim_streamed(ellhip_batch *spaces, ellhip_batch_svm *o, double *gamma_inout, int64_t max_iters,
                                    double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                                    int32_t *status_out);
/* The same on a streamed EllStable handle (variant ELLHIP_SPACE_ELL_STABLE); a streamed Ell handle is refused. */
int ellhip_batch_svm_optim_streamed_stable(ellhip_batch *spaces, ellhip_batch_svm *o, double *gamma_inout,
                                           int64_t max_iters, double tol, double *x_best_out, int32_t *has_best_out,
                                           int64_t *niter_out, int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif
