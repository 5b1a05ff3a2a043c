/*
 * ellhip_lmi_loop.h -- C ABI of the round-robin problem handle over large LMI blocks (ellhip_lmi.h, m <= 8192) and
 * of the device-resident cutting-plane loops built on it (libellhip.so).
 *
 * The oracle is the one of tests/lmi_tests.rs:142-171 generalised to J blocks and an optional objective:
 *     min c'x  s.t.  F_j(x) > 0, j = 0 .. J-1          (with c: the optimisation form)
 *     find x   s.t.  F_j(x) > 0                        (without c: the feasibility form)
 * A call walks the stations behind the cursor `idx`, wrapping: the J blocks (each one call of the block's own
 * oracle, ellhip_lmi_assess_feas) and, in the optimisation form, station J, the objective: f0 = c.x as a left fold
 * from 0.0 in ascending k; the cut (c, f0 - gamma) when f0 - gamma > 0, else gamma = f0 and the walk goes on.  The
 * walk ends at the first cut.  `station` names what it ended on:
 *     station <  J      that block cut (gradient and ep of the block's LDLT witness)
 *     station == J      the objective cut
 *     station == J + 1  every station passed: the cut (c, 0.0), meant as a central cut ("shrunk")
 * The feasibility form walks the J blocks only; when all pass there is no cut.
 *
 * Everything is decided on the device.  One iteration is a fixed window of station slots that covers every
 * cyclic walk (2J + 1 slots with an objective, 2J - 1 without; one slot for a single-block feasibility handle),
 * issued as ordinary kernel launches on one stream.  A slot that is not the walk's next station runs as empty
 * launches (every kernel of the block's call returns at once).  The host looks at the device once per 64
 * iterations.  The results are bit-identical to the same loop driven from the host through
 * ellhip_lmi_assess_feas and ellhip_update.
 *
 * Which form is faster (one MI355X, 200 iterations, against the host-driven loop from a compiled caller; DESIGN.md
 * section 10.1, profiles/lmi/device_loop.jsonl).  A single-block feasibility handle has one slot and no skipped
 * launches: the device loop is the faster form at every size measured, 1.85 times the host-driven rate at
 * (n, m) = (16, 64), 1.34 at (24, 300), 1.28 at (8, 2048).  With two blocks and an objective the window has five
 * slots of which a walk uses one to three, and the device loop was the SLOWER form at every shape measured: 0.78
 * of the host-driven rate at (8, 70), 0.96 at (24, 300), 0.94 at (8, 1057).  There is no m from which downwards
 * the multi-block form wins: drive such a problem from the host (RoundRobinLmiHost in lmi_loop_hip.hpp) unless the
 * host has to stay free.
 *
 * Same conventions as ellhip.h: host buffers owned by the caller, plain pointers and sizes, 0 = ok,
 * negative = ELLHIP_E_*, no CPU fallback.
 */
#ifndef ELLHIP_LMI_LOOP_H
#define ELLHIP_LMI_LOOP_H

#include "ellhip.h"
#include "ellhip_lmi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellhip_lmi_loop ellhip_lmi_loop;
#define ELLHIP_LMI_LOOP_JMAX 8

/* J block oracles (borrowed: the caller keeps them alive, and does not call them while a loop call is running),
 * all with the same n >= 1 on the same device; the m_j may differ; LMIOracle and LMI0Oracle blocks may be mixed.
 * c[n]: the objective of the optimisation form, or NULL for the feasibility form.
 * ELLHIP_E_INVALID: J outside 1 .. ELLHIP_LMI_LOOP_JMAX, a NULL block, a block with n == 0 (the bare LDLTMgr
 * form), blocks that differ in n or device.  ELLHIP_E_NODEVICE without a HIP device. */
int ellhip_lmi_loop_create(ellhip_lmi_loop **out, ellhip_lmi *const *blocks, int64_t J, const double *c);
void ellhip_lmi_loop_destroy(ellhip_lmi_loop *o);

/* The round-robin cursor: the station visited last, -1 when new.  set_idx accepts -1 .. J with an objective and
 * -1 .. J - 1 without. */
int ellhip_lmi_loop_get_idx(ellhip_lmi_loop *o, int *idx_out);
int ellhip_lmi_loop_set_idx(ellhip_lmi_loop *o, int idx);

/* One oracle call at a host point x[n], run on the device exactly as an iteration of the loops runs it.
 * assess_optim (handle created with c, else ELLHIP_E_INVALID): always a cut, returns 1; g_out[n], *beta_out,
 * *station_out as above, *gamma_inout receives the new gamma.
 * assess_feas (handle created without c, else ELLHIP_E_INVALID): returns 1 with a cut, 0 when every block passed
 * (g_out and *beta_out are then left alone and *station_out is -1).
 * Afterwards ellhip_lmi_pos / _get_witness / _get_storage of every block report that block's last executed call. */
int ellhip_lmi_loop_assess_optim(ellhip_lmi_loop *o, const double *x, double *gamma_inout, double *g_out,
                                 double *beta_out, int *station_out);
int ellhip_lmi_loop_assess_feas(ellhip_lmi_loop *o, const double *x, double *g_out, double *beta_out,
                                int *station_out);

/* cutting_plane_optim (src/cutting_plane.rs:286-313) / cutting_plane_feas (:205-227) with omega = this handle and
 * space = an UNSHARDED ellhip_space (Ell at any defer depth, or EllStable) of dimension n on the handle's device,
 * run entirely on the device.  ELLHIP_E_INVALID for a space whose n or device differs, a sharded space,
 * max_iters < 0, and for the wrong form of handle (optim needs c, feas needs none); a refused call changes nothing.
 * optim: x_best_out[n] (written when *has_best_out), *niter_out and *gamma_inout are the reference's (x_best, niter)
 * and gamma.  feas: x_out[n] is written when *feasible_out, and left alone otherwise.  The space is left in the
 * state the reference loop leaves it in, the cursor where the last walk left it. */
int ellhip_lmi_loop_optim(ellhip_space *s, ellhip_lmi_loop *o, double *gamma_inout, int64_t max_iters, double tol,
                          double *x_best_out, int *has_best_out, int64_t *niter_out);
int ellhip_lmi_loop_feas(ellhip_space *s, ellhip_lmi_loop *o, int64_t max_iters, double tol, double *x_out,
                         int *feasible_out, int64_t *niter_out);

#ifdef __cplusplus
}
#endif
#endif
