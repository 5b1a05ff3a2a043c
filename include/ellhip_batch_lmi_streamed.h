/*
 * ellhip_batch_lmi_streamed.h -- C ABI of the batched, device-resident LMI cutting-plane loops on streamed batch handles
 * (libellhip.so).
 *
 * ellhip_batch_lmi.h solves B independent LMI-constrained problems of one shape (n variables, J blocks of size m_j) on the
 * batch engine that keeps each matrix in LDS, so it stops at n = 128, and the matrix shares the workgroup's LDS with the
 * m x m factorisation (n = 128 only with M = max m_j <= 8); ellhip_batch_stable_loops.h does the same on EllStable spaces.
 * This header carries both solves to every shape n <= 1024, J <= 8, m_j <= 64: the spaces are a streamed batch handle
 * (ellhip_batch_streamed.h for Ell, ellhip_batch_streamed_stable.h for EllStable: the matrices stay in HBM, one workgroup
 * per ellipsoid, one thread per row) and one kernel per chunk of iterations runs `cutting_plane_optim`
 * (src/cutting_plane.rs:286-313) or `cutting_plane_feas` (:205-227) for every problem -- the round-robin oracle of
 * tests/lmi_tests.rs:142-171 over `LMIOracle` / `LMI0Oracle` (src/oracles/lmi_oracle.rs:26-44, lmi0_oracle.rs:16-34) and
 * `LDLTMgr::factor / witness / sym_quad` (src/oracles/ldlt_mgr.rs:29-55, 98-124), x_best, the update (src/ell.rs:96-128 or
 * EllStable::update_core, src/ell_stable.rs:52-125) and the stop test -- with no host in the loop.  The oracle is the device
 * function ellhip_batch_lmi.h runs.  Cuts, stations, iteration counts, x_best / x, gamma, idx and the spaces afterwards
 * (matrix, xc, kappa, tsq; EllStable's scratch triangle included) are bit-identical to the CPU arithmetic and, at n <= 128,
 * to ellhip_batch_lmi_optim / _feas / _optim_stable / _feas_stable on an LDS handle.
 *
 * The oracle handle is an ordinary ellhip_batch_lmi: _destroy, _assess_optim, _get_idx, _set_idx and _set_chunk of
 * ellhip_batch_lmi.h work on it at every n (past n = 128 _assess_optim runs one workgroup of n threads, rounded up to whole
 * waves, per problem, with 8 * (((2 n + M * (M | 1) + M + 16) | 1) + n) bytes of LDS: 57.1 KiB at n = 1024, M = 64).
 *
 * Memory: the pencil is kept k-fastest on the device, 8 * n * sum m_j^2 bytes per pencil; one pencil when shared_f, B
 * otherwise (32 MiB each at n = 1024, J = 1, m = 64), and beside it the copy of its lower triangles that F(x) reads (below),
 * 4 * n * sum m_j (m_j + 1) bytes.  Pencils that are not shared are repacked and uploaded one problem at
 * a time, so the constructor holds one repacked pencil on the host, not B.  A set of pencils above 100e9 bytes as stored is
 * refused with ELLHIP_E_NOMEM.
 *
 * Traffic per problem and round: 16 n^2 bytes of matrix on Ell (the product of round k + 1 rides on the sweep of round k
 * whenever round k + 1 has a gradient; the first round of a launch adds 8 n^2) or 24 n^2 on EllStable (nothing is fused: the
 * centre is final only after the back solve); for the oracle, per visited block 4 m (m + 1) n bytes of pencil for F(x) and,
 * on a cut whose factorisation stopped at row p, 8 (p + 1)^2 n bytes for the n quadratic forms.  One visit of a 64 x 64
 * block reads 16 640 n bytes, as much as an Ell sweep at n = 1040; a pencil shared by every problem (32 + 16 MiB at
 * n = 1024, m = 64) fits the Infinity Cache.
 *
 * LDS per workgroup, with e(n) = n rounded up to even and M = max m_j:
 *
 *     Ell:        8 * (5 e(n) + 8  + ((2 n + M * (M | 1) + M + 16) | 1)) bytes, 89.2 KiB at n = 1024, M = 64;
 *     EllStable:  8 * (4 e(n) + 72 + ((2 n + M * (M | 1) + M + 16) | 1)) bytes, 81.7 KiB at n = 1024, M = 64.
 *
 * Above 64 KiB the drivers opt in per kernel and device (hipFuncAttributeMaxDynamicSharedMemorySize, raised only); the
 * limit is the 159 KiB of ellhip_batch_lmi.h, which no shape of this header reaches, so no shape is refused for LDS.  At
 * n = 512, M = 64 the Ell loop needs 61.2 KiB, so two workgroups share a CU's 160 KiB where the low-pass loop has three.
 * Compiled for gfx950 and bounded for 1024 threads (128 VGPRs a wave) the two loop kernels take 103 (Ell) and 109
 * (EllStable) VGPRs and the wide oracle call 62, none with scratch.
 *
 * F(x): beside the k-fastest pencil the handle keeps the lower triangles element-fastest, [block][k][t] with
 * t = a (a + 1) / 2 + b (half the pencil's size again, counted by the cap), and thread i folds the elements t = i, i + n, ...
 * from it: coalesced loads, the same fold per element, the same bits.  Measured against F(x) from the k-fastest pencil
 * (whole calls, M = 64, shared pencil): 85 ms against 114 ms for 40 rounds at (n, B) = (256, 1536), 30 ms against 35 ms for
 * 12 rounds at (1024, 252).
 *
 * Measured on one MI355X (tools/batch_lmi_streamed_bench.py; whole calls, rounds per second of all
 * problems together, one M x M block, a mix of starts inside and outside the feasible set, M = 8 / 64): with one shared
 * pencil on Ell at (n, B) = (129, 1536) 1.34e7 / 9.6e5, (256, 1536) 4.4e6 / 7.2e5, (512, 768) 1.03e6 / 3.2e5, (1024, 252)
 * 2.1e5 / 1.0e5, which is 6.5 ... 1.48 times the host-driven form (one wide ellhip_batch_lmi_assess_optim and one
 * ellhip_batch_update per iteration) and 0.92 ... 0.04 of the engine's own update rate at K = 8 cuts per launch; on
 * EllStable at B = 1536 / 510 / 510 / 510: 4.3e6 / 8.1e5, 1.07e6 / 3.6e5, 3.0e5 / 1.8e5, 4.5e4 / 3.6e4, which is
 * 2.7 ... 1.13 times and 0.95 ... 0.15.  With per-problem pencils (B lowered to 672 ... 84 at M = 64 by the tool's 4 GiB cap)
 * 1.03e7 ... 1.2e4 rounds/s, 5.2 ... 1.12 times the host-driven form.  Against the CPU loop on one thread (timed once, from
 * Python, on a shared host) 150 ... 2450 times.  With a 64-block the oracle is most of a round (0.66 ... 0.98 of it on Ell,
 * 0.23 ... 0.91 on EllStable).  The device loop was faster than the host-driven form at every shape measured; on EllStable at
 * n = 1024, where the serial back solve sets the pace, by 12 ... 15 per cent only, against a baseline timed once.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_LMI_STREAMED_H
#define ELLHIP_BATCH_LMI_STREAMED_H

#include "ellhip_batch_lmi.h"
#include "ellhip_batch_streamed.h"
#include "ellhip_batch_streamed_stable.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ellhip_batch_lmi_create for 1 <= n <= ELLHIP_BATCH_STREAMED_NMAX (1024); every other argument and refusal as there,
 * checked before the device and in the same order.  shared_f = 0: mat_f as there, [B][n][m_j][m_j] per block, blocks
 * concatenated in j.  shared_f != 0: mat_f is [n][m_j][m_j] per block, one pencil that all B problems read; mat_b
 * ([B][m_j][m_j] per block, or NULL) and c ([B][n], or NULL) stay per problem. */
int ellhip_batch_lmi_create_streamed(ellhip_batch_lmi **out, int64_t B, int64_t n, int64_t J, const int64_t *m,
                                     const double *mat_f, int32_t shared_f, const double *mat_b, const double *c, int device);

/* ellhip_batch_lmi_optim on a streamed handle: same arguments, semantics and outputs.  spaces must be a streamed batch
 * handle (ellhip_batch_is_streamed) of Ell spaces with the oracle's B, n and device; a streamed handle of n <= 128 is
 * accepted.  Anything else -- an LDS handle, a streamed EllStable handle, a mismatch, a NULL argument, an oracle handle
 * made without c -- is ELLHIP_E_INVALID with a message, and the spaces, idx and outputs are left untouched. */
int ellhip_batch_lmi_optim_streamed(ellhip_batch *spaces, ellhip_batch_lmi *o, double *gamma_inout, int64_t max_iters,
                                    double tol, double *x_best_out, int32_t *has_best_out, int64_t *niter_out,
                                    int32_t *status_out);
/* ellhip_batch_lmi_feas on a streamed Ell handle; refuses what _optim_streamed refuses, and an oracle handle made with c. */
int ellhip_batch_lmi_feas_streamed(ellhip_batch *spaces, ellhip_batch_lmi *o, int64_t max_iters, double tol, double *x_out,
                                   int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);
/* The same two on a streamed EllStable handle (variant ELLHIP_SPACE_ELL_STABLE); a streamed Ell handle is refused. */
int ellhip_batch_lmi_optim_streamed_stable(ellhip_batch *spaces, ellhip_batch_lmi *o, double *gamma_inout,
                                           int64_t max_iters, double tol, double *x_best_out, int32_t *has_best_out,
                                           int64_t *niter_out, int32_t *status_out);
int ellhip_batch_lmi_feas_streamed_stable(ellhip_batch *spaces, ellhip_batch_lmi *o, int64_t max_iters, double tol,
                                          double *x_out, int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif
