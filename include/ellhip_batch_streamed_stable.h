/*
 * ellhip_batch_streamed_stable.h -- C ABI of the streamed batch engine for EllStable (libellhip.so).
 *
 * B independent `EllStable` search spaces (src/ell_stable.rs:9-15) of one dimension n <= 1024 behind one ellhip_batch
 * handle: the EllStable counterpart of ellhip_batch_streamed.h, as ellhip_batch_create_stable is that of
 * ellhip_batch_create.  The packed buffers stay in HBM and are streamed through the update, one workgroup per ellipsoid,
 * one thread per index.
 *
 * The handle is an ordinary ellhip_batch of variant ELLHIP_SPACE_ELL_STABLE for which ellhip_batch_is_streamed returns 1.
 * Every ellhip_batch_* entry point of ellhip_batch.h (_update, _update_dev, _synchronize, _stream, the four getters,
 * _set_xc, _size, _ndim, _variant, _set_use_parallel_cut, _destroy) works on it with the semantics of a handle made by
 * ellhip_batch_create_stable; _set_no_defer_trick returns ELLHIP_E_INVALID, as on any EllStable batch.  Every step follows
 * EllStable::update_core (src/ell_stable.rs:52-125) statement for statement, so the results are bit-identical to the CPU
 * arithmetic and to the LDS engine, the scratch triangle included: ellhip_batch_get_mq returns each packed buffer exactly
 * as the reference would hold it (diagonal = D, strict upper = the factor, strict lower = scratch).  Inside the handle the
 * scratch triangle is kept in another order; the constructors and ellhip_batch_get_mq convert, nothing else shows it.
 *
 * Of the batched cutting-plane loops the low-pass one runs on such a handle, through entry points of its own
 * (ellhip_batch_lowpass_streamed_stable.h).  Every other loop entry point refuses it with ELLHIP_E_INVALID and leaves it
 * untouched: the loops of ellhip_batch_{lmi,lowpass,svm}.h, their _stable forms and
 * ellhip_batch_lowpass_{optim,feas}_streamed.
 *
 * Traffic per ellipsoid, what the kernel moves: a cut reads the factor once for the forward solve (4 n^2 bytes) and writes
 * the scratch triangle (4 n^2); a successful cut reads the scratch triangle twice more (8 n^2) and reads and writes the
 * factor (8 n^2): 24 n^2 bytes, 8 n^2 for a cut that fails.  The back solve of a successful cut is a chain of n (n-1) / 2
 * dependent subtractions, as in the reference; throughput comes from the number of ellipsoids in flight.
 *
 * Not offered: n > 1024, sharding.  Same conventions as ellhip.h: 0 = ok, negative = ELLHIP_E_*, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_STREAMED_STABLE_H
#define ELLHIP_BATCH_STREAMED_STABLE_H

#include "ellhip_batch_streamed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* B EllStable spaces of dimension n, 1 <= n <= ELLHIP_BATCH_STREAMED_NMAX, with the arguments of ellhip_batch_create_stable:
 * kappa B values or NULL = 1.0; mq B*n*n packed buffers, row-major, taken verbatim (the strict lower triangle comes back
 * unchanged from ellhip_batch_get_mq until the first update overwrites it), or NULL with diag B*n, or both NULL = identity;
 * xc B*n or NULL = 0.  ELLHIP_E_INVALID for B < 1 or n outside 1..1024, ELLHIP_E_NODEVICE without a device. */
int ellhip_batch_create_streamed_stable(ellhip_batch **out, int64_t B, int64_t n, const double *kappa, const double *mq,
                                        const double *diag, const double *xc, int device);
/* B clones of one unsharded EllStable handle of dimension <= 1024, as ellhip_batch_stable_from_space: each clone's
 * ellhip_batch_get_mq equals the handle's ellhip_get_mq bit for bit.  Ell handles are refused. */
int ellhip_batch_streamed_stable_from_space(ellhip_batch **out, const ellhip_space *space, int64_t B);

#ifdef __cplusplus
}
#endif
#endif
