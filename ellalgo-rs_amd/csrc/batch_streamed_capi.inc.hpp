// batch_streamed_capi.inc.hpp -- C ABI of the streamed batch engine (include/ellhip_batch_streamed.h).  Included from
// ellhip_capi.hip right after batch_capi.inc.hpp: the handle is that file's ellhip_batch with `streamed` set, and every
// ellhip_batch_* entry point there reaches the kernel here through batch_shape / batch_launch.
#include "../../include/ellhip_batch_streamed.h"

static_assert(ELLHIP_BATCH_STREAMED_NMAX == ellhip::BATCH_STREAMED_NMAX, "header and kernel disagree on the largest n");

namespace {

// one workgroup per ellipsoid, one thread per row: n rounded up to whole waves
int batch_streamed_shape(ellhip_batch* h) {
    h->T = (h->n + 63) / 64 * 64;
    h->epw = 1;
    h->lds_bytes = batch_streamed_lds_doubles(h->n) * sizeof(double);  // at most 40 KiB: no opt-in needed
    return 0;
}

int batch_streamed_launch(ellhip_batch* h, long long K, const int* kinds, const double* grads, const double* b0, const int* hb1,
                          const double* b1, int* status, double* tsq_out) {
    BatchStreamedParams P;
    P.B = h->B;
    P.n = h->n;
    P.np = batch_streamed_np(h->n);
    P.K = (int)K;
    P.no_defer_trick = h->no_defer_trick;
    const EllCalcDev calc = EllCalcDev::make(h->n, h->use_parallel_cut);
    hipLaunchKernelGGL(k_batch_streamed_update, dim3((unsigned)h->B), dim3(h->T), h->lds_bytes, h->stream, P, h->d_Q, h->d_xc,
                       h->d_kappa, h->d_tsq, h->d_sym, kinds, grads, b0, hb1, b1, status, tsq_out, calc);
    HIPCHK(hipGetLastError());
    return 0;
}

// sym[b] for matrices that came from outside (compared bit by bit), or 1 everywhere for identity / diag
int batch_streamed_flags(ellhip_batch* h, bool compare) {
    if (compare)
        hipLaunchKernelGGL(k_bs_symcheck, dim3((unsigned)h->B), dim3(256), 0, h->stream, (const double*)h->d_Q, h->n, h->d_sym);
    else
        hipLaunchKernelGGL(k_bs_fill_int, dim3(256), dim3(256), 0, h->stream, h->d_sym, h->B, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

}  // namespace

extern "C" {

int ellhip_batch_create_streamed(ellhip_batch** out, int64_t B, int64_t n, const double* kappa, const double* mq,
                                 const double* diag, const double* xc, int device) {
    int rc = batch_create(out, B, n, kappa, mq, diag, xc, device, ELLHIP_SPACE_ELL, true);
    if (rc) return rc;
    DeviceGuard guard((*out)->device);
    rc = batch_streamed_flags(*out, mq != nullptr);
    if (rc) {
        ellhip_batch_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

int ellhip_batch_streamed_from_space(ellhip_batch** out, const ellhip_space* space_c, int64_t B) {
    if (ellhip_device_count() <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched engine has no CPU path");
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!space_c) return fail(ELLHIP_E_INVALID, "NULL handle");
    ellhip_space* s = const_cast<ellhip_space*>(space_c);
    if (s->variant != ELLHIP_SPACE_ELL || s->sharded)
        return fail(ELLHIP_E_INVALID, "streamed batch engine: clones of an unsharded Ell only");
    int rc = batch_clone_space(out, s, B, true);
    if (rc) return rc;
    DeviceGuard guard((*out)->device);
    rc = batch_streamed_flags(*out, true);
    if (rc) {
        ellhip_batch_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

int ellhip_batch_is_streamed(const ellhip_batch* h) {
    if (!h) {
        if (ellhip_device_count() <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched engine has no CPU path");
        return fail(ELLHIP_E_INVALID, "NULL handle");
    }
    return h->streamed;
}

}  // extern "C"
