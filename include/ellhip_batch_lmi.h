/*
 * ellhip_batch_lmi.h -- C ABI of the batched, device-resident cutting-plane loop for LMI-constrained problems
 * (libellhip.so).
 *
 * B independent problems of one shape, for b = 0..B-1 with n <= 128 variables and J blocks (block j of size m_j):
 *
 *     minimise c_b' x   subject to   B_bj - sum_k x_k F_bjk > 0   for j = 0..J-1          (mat_b given)
 *                                          sum_k x_k F_bjk > 0                             (mat_b == NULL)
 *
 * Each block is an `LMIOracle` (src/oracles/lmi_oracle.rs:26-44) or, without mat_b, an `LMI0Oracle`
 * (src/oracles/lmi0_oracle.rs:16-34), both on `LDLTMgr::factor / witness / sym_quad` (src/oracles/ldlt_mgr.rs:29-55,
 * 98-124).  They are combined by the round-robin optimisation oracle of tests/lmi_tests.rs:142-171 generalised from two
 * blocks to J: an index `idx` per problem starts at -1 and persists across calls; a call folds f0 = c . x left to right
 * from 0.0, then visits at most J + 1 stations in cyclic order after idx.  Stations 0..J-1 are `assess_feas` of that
 * block (a cut (g, ep) ends the call), station J is the objective (fj = f0 - gamma; a cut (c, fj) if fj > 0, else
 * gamma = f0).  When every station passes, the call answers ((c, 0.0), true).  J = 2 with the reference's matrices is
 * `MyLmiOracle`.
 *
 * The loop entry points run `cutting_plane_optim` (src/cutting_plane.rs:286-313) or `cutting_plane_feas` (:205-227) for
 * every problem on the device: one workgroup-resident ellipsoid per problem (an ellhip_batch handle of `Ell` spaces),
 * oracle and update in the same kernel, no host in the loop.  All arithmetic is + - * / in the reference's fold order,
 * so iteration counts, x_best, gamma and the spaces afterwards are bit-identical to the CPU arithmetic.
 *
 * `EllStable` batch handles belong to ellhip_batch_stable_loops.h (ellhip_batch_lmi_optim_stable, _feas_stable): the loop
 * entry points here refuse them with ELLHIP_E_INVALID.  Problems of up to 1024 variables and streamed batch handles belong
 * to ellhip_batch_lmi_streamed.h; the entry points of this header keep refusing both.
 *
 * LDS: a workgroup holds `epw` problems, epw as the batch engine chooses it for n (ellhip_batch.h).  With
 * p(k) = k | 1 and M = max_j m_j it needs
 *
 *     epw * 8 * ( ((n * p(n) + 2 n + 8) | 1)  +  ((2 n + M * p(M) + M + 16) | 1) )   bytes,
 *
 * the first term being the batch engine's own (matrix, gradient, Q g, scalars), the second the oracle's (x, c, the
 * m x m factorisation, the witness, scalars).  A shape that needs more than 159 KiB (the device's 160 KiB per workgroup
 * less 1 KiB the kernel keeps for itself) is refused by the loop entry points; n = 128 fits with M <= 8, n <= 64 with
 * every M <= 64.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, 0 = ok, negative = ELLHIP_E_*, ELLHIP_E_NODEVICE
 * without a device, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_LMI_H
#define ELLHIP_BATCH_LMI_H

#include "ellhip_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellhip_batch_lmi ellhip_batch_lmi;
#define ELLHIP_BATCH_LMI_JMAX 8
#define ELLHIP_BATCH_LMI_MMAX 64

/* m: [J].  mat_f: for block j an array [B][n][m_j][m_j] (LMIOracle::new's mat_f per problem, src/oracles/lmi_oracle.rs:12),
 * blocks concatenated in j.  mat_b: [B][m_j][m_j] per block, concatenated, or NULL (LMI0 form, src/oracles/lmi0_oracle.rs:10).
 * c: [B][n], or NULL (feasibility problem: no objective station). */
int ellhip_batch_lmi_create(ellhip_batch_lmi **out, int64_t B, int64_t n, int64_t J, const int64_t *m,
                            const double *mat_f, const double *mat_b, const double *c, int device);
void ellhip_batch_lmi_destroy(ellhip_batch_lmi *o);

/* One oracle call (assess_optim, tests/lmi_tests.rs:145-171) for every problem at x[B][n]; advances idx.
 * station_out[B] = the station that produced the cut (J = objective cut, J+1 = "shrunk": every station passed),
 * grad_out[B][n], beta_out[B], gamma_inout[B].  On a handle made without c the stations are the J blocks only
 * (J+1 = feasible; grad_out of such a problem is left untouched). */
int ellhip_batch_lmi_assess_optim(ellhip_batch_lmi *o, const double *x, double *gamma_inout, double *grad_out,
                                  double *beta_out, int32_t *station_out);
int ellhip_batch_lmi_get_idx(ellhip_batch_lmi *o, int32_t *idx_out);   /* [B] */
int ellhip_batch_lmi_set_idx(ellhip_batch_lmi *o, const int32_t *idx); /* NULL = -1 each */

/* cutting_plane_optim (src/cutting_plane.rs:286-313) for every problem, on the device.  spaces: an Ell batch handle with
 * the same B, n, device.  gamma_inout[B]; x_best_out[B][n] (rows with has_best_out[b] == 0 untouched); niter_out[B];
 * status_out[B] = the CutStatus of the last update (Success when the tolerance or max_iters ended the loop).
 * Afterwards the spaces and idx are in the state the reference loop leaves them in (the update that hit the tolerance
 * is complete), so ellhip_batch_update, the getters and a second call continue from there. */
int ellhip_batch_lmi_optim(ellhip_batch *spaces, ellhip_batch_lmi *o, double *gamma_inout, int64_t max_iters, double tol,
                           double *x_best_out, int32_t *has_best_out, int64_t *niter_out, int32_t *status_out);
/* cutting_plane_feas (src/cutting_plane.rs:205-227) with the J blocks as round-robin stations: x_out[b] = the first xc
 * that passes all of them (feasible_out[b] = 1, status Success), rows of infeasible problems untouched. */
int ellhip_batch_lmi_feas(ellhip_batch *spaces, ellhip_batch_lmi *o, int64_t max_iters, double tol,
                          double *x_out, int32_t *feasible_out, int64_t *niter_out, int32_t *status_out);
/* iterations per launch (default 256, 1..4096): the host looks at the "all stopped" count between launches */
int ellhip_batch_lmi_set_chunk(ellhip_batch_lmi *o, int64_t iters);

#ifdef __cplusplus
}
#endif
#endif
