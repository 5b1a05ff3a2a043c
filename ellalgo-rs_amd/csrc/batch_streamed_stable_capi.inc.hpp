// batch_streamed_stable_capi.inc.hpp -- C ABI of the streamed batch engine for EllStable
// (include/ellhip_batch_streamed_stable.h).  Included from ellhip_capi.hip right after batch_streamed_capi.inc.hpp: the
// handle is batch_capi.inc.hpp's ellhip_batch with `streamed` set and variant ELLHIP_SPACE_ELL_STABLE, and every
// ellhip_batch_* entry point there reaches the kernel here through batch_shape / batch_launch; ellhip_batch_get_mq goes
// through batch_streamed_stable_rotate around its copy.
#include "../../include/ellhip_batch_streamed_stable.h"

#include "batch_streamed_stable_kernels.hpp"

namespace {

// one workgroup per ellipsoid, one thread per index: n rounded up to whole waves
int batch_streamed_stable_shape(ellhip_batch* h) {
    h->T = (h->n + 63) / 64 * 64;
    h->epw = 1;
    h->lds_bytes = batch_streamed_stable_lds_doubles(h->n) * sizeof(double);  // at most 24.6 KiB: no opt-in needed
    return 0;
}

int batch_streamed_stable_launch(ellhip_batch* h, long long K, const int* kinds, const double* grads, const double* b0,
                                 const int* hb1, const double* b1, int* status, double* tsq_out) {
    BatchStreamedParams P;
    P.B = h->B;
    P.n = h->n;
    P.np = batch_streamed_np(h->n);
    P.K = (int)K;
    P.no_defer_trick = 0;
    const EllCalcDev calc = EllCalcDev::make(h->n, h->use_parallel_cut);
    hipLaunchKernelGGL(k_batch_streamed_update_stable, dim3((unsigned)h->B), dim3(h->T), h->lds_bytes, h->stream, P, h->d_Q,
                       h->d_xc, h->d_kappa, h->d_tsq, kinds, grads, b0, hb1, b1, status, tsq_out, calc);
    HIPCHK(hipGetLastError());
    return 0;
}

// the reference's packed buffers <-> the engine's, in place on the handle's stream (the map is its own inverse)
int batch_streamed_stable_rotate(ellhip_batch* h) {
    if (h->n < 3) return 0;  // no scratch element moves
    const unsigned tiles = (unsigned)((h->n + BSS_TILE - 1) / BSS_TILE);
    const unsigned gx = (unsigned)std::min<long long>(h->B, 1 << 16);
    hipLaunchKernelGGL(k_bss_rotate, dim3(gx, tiles, tiles), dim3(256), 0, h->stream, h->d_Q, h->B, h->n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int batch_streamed_stable_finish(ellhip_batch** out, bool rotate) {
    if (!rotate) return 0;
    DeviceGuard guard((*out)->device);
    const int rc = batch_streamed_stable_rotate(*out);
    if (rc) {
        ellhip_batch_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

}  // namespace

extern "C" {

int ellhip_batch_create_streamed_stable(ellhip_batch** out, int64_t B, int64_t n, const double* kappa, const double* mq,
                                        const double* diag, const double* xc, int device) {
    const int rc = batch_create(out, B, n, kappa, mq, diag, xc, device, ELLHIP_SPACE_ELL_STABLE, true);
    if (rc) return rc;
    return batch_streamed_stable_finish(out, mq != nullptr);  // identity / diag: the scratch triangle is all zeros
}

int ellhip_batch_streamed_stable_from_space(ellhip_batch** out, const ellhip_space* space_c, int64_t B) {
    if (ellhip_device_count() <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched engine has no CPU path");
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!space_c) return fail(ELLHIP_E_INVALID, "NULL handle");
    ellhip_space* s = const_cast<ellhip_space*>(space_c);
    if (s->variant != ELLHIP_SPACE_ELL_STABLE || s->sharded)
        return fail(ELLHIP_E_INVALID, "streamed batch engine: clones of an unsharded EllStable only");
    const int rc = batch_clone_space(out, s, B, true);
    if (rc) return rc;
    return batch_streamed_stable_finish(out, true);
}

}  // extern "C"
