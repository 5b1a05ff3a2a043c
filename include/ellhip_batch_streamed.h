/*
 * ellhip_batch_streamed.h -- C ABI of the streamed batch engine (libellhip.so).
 *
 * B independent `Ell` search spaces (src/ell.rs:9-16) of one dimension n <= 1024 behind one ellhip_batch handle.  The
 * batched engine of ellhip_batch.h keeps each matrix in LDS and therefore stops at n = 128; here the matrices stay in HBM
 * and are streamed through the update, one workgroup per ellipsoid, one thread per row.  It covers the reference's
 * mid-size usage -- `BSearchAdaptor::assess_bs` clones (src/cutting_plane.rs:403-419), parameter sweeps and FIR lengths of
 * a few hundred taps -- where one ellipsoid still cannot fill a GPU and the single-handle engine is bound by its launches.
 *
 * The handle is an ordinary ellhip_batch of variant ELLHIP_SPACE_ELL: every ellhip_batch_* entry point of ellhip_batch.h
 * (_update, _update_dev, _synchronize, _stream, the four getters, _set_xc, _size, _ndim, _variant, _set_no_defer_trick,
 * _set_use_parallel_cut, _destroy) works on it with unchanged semantics, and ellhip_batch_get_mq returns each matrix
 * exactly as the reference would hold it (before the first successful cut that includes a non-symmetric upper triangle).
 * Every step follows the reference's statement order, so the results are bit-identical to the CPU arithmetic and to the
 * LDS engine.  The batched cutting-plane loops of ellhip_batch_{lmi,lowpass,svm}.h and their _stable forms refuse a
 * streamed handle with ELLHIP_E_INVALID at every n: their kernel assumes the LDS layout.  The low-pass design loop has
 * entry points of its own for a streamed handle, ellhip_batch_lowpass_{optim,feas}_streamed (ellhip_batch_lowpass_streamed.h).
 *
 * Traffic per ellipsoid, what the kernel moves: the first cut of a launch, or a cut that follows a failed one, reads the
 * matrix once for Q g (8 n^2 bytes) and a successful cut reads and writes it once more for the rank-1 update (16 n^2);
 * a cut that follows a successful one in the same launch finds its Q g folded into that update's sweep and costs 16 n^2
 * alone.  K successful cuts in one launch: (16 K + 8) n^2 bytes, that is 24 n^2 at K = 1 and 17 n^2 per cut at K = 8.
 * A matrix given by the caller that is not symmetric to the bit is read along its true rows (uncoalesced, slower) until
 * its first successful cut has mirrored it.
 *
 * EllStable on this engine: ellhip_batch_streamed_stable.h.  Not offered: n > 1024, sharding.  Same conventions as
 * ellhip.h: 0 = ok, negative = ELLHIP_E_*, no CPU fallback.
 */
#ifndef ELLHIP_BATCH_STREAMED_H
#define ELLHIP_BATCH_STREAMED_H

#include "ellhip_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ELLHIP_BATCH_STREAMED_NMAX 1024

/* B ellipsoids of dimension n, 1 <= n <= 1024, with the arguments of ellhip_batch_create: kappa B values or NULL = 1.0;
 * mq B*n*n dense row-major, taken verbatim (need not be symmetric), or NULL with diag B*n, or both NULL = identity;
 * xc B*n or NULL = 0.  ELLHIP_E_INVALID for B < 1 or n outside 1..1024, ELLHIP_E_NODEVICE without a device. */
int ellhip_batch_create_streamed(ellhip_batch **out, int64_t B, int64_t n, const double *kappa, const double *mq,
                                 const double *diag, const double *xc, int device);
/* B clones of one unsharded Ell handle of dimension <= 1024, as ellhip_batch_from_space.  EllStable handles are refused. */
int ellhip_batch_streamed_from_space(ellhip_batch **out, const ellhip_space *space, int64_t B);
/* 1 for a handle made by one of the two constructors above or by those of ellhip_batch_streamed_stable.h, 0 for any other
 * batch handle; negative = ELLHIP_E_* */
int ellhip_batch_is_streamed(const ellhip_batch *h);

#ifdef __cplusplus
}
#endif
#endif
