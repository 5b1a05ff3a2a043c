// batch_svm_capi.inc.hpp -- C ABI of the batched device-resident SVM cutting-plane loop (include/ellhip_batch_svm.h).
// Included at the end of ellhip_capi.hip, after batch_capi.inc.hpp (it drives the batch engine's handle directly) and
// batch_lmi_capi.inc.hpp (batch_lmi_allow_lds, BATCH_LMI_LDS_MAX).
//
// Reference: src/oracles/svm_oracle.rs:4-58 (oracle), src/cutting_plane.rs:286-313 (loop).
#include "../../include/ellhip_batch_svm.h"

#include "batch_svm_kernels.hpp"

struct ellhip_batch_svm {
    int device = 0;
    long long B = 0;
    int m = 0;
    int nfeat = 0;
    int n = 0;                    // nfeat + 1
    long long ld = 0;             // m rounded up to 8 doubles
    int shared = 0;
    int chunk = 256;
    double* d_XT = nullptr;       // [ntab][nfeat][ld], ntab = 1 (shared) or B
    int* d_labels = nullptr;      // [B][m]
    long long* d_minidx = nullptr;  // [B]
    double* d_minval = nullptr;   // [B]
    double* d_gamma = nullptr;    // [B]
    double* d_xbest = nullptr;    // [B][n]
    long long* d_niter = nullptr; // [B]
    int* d_ints = nullptr;        // has_best [B], stopped [B], status [B], nstopped [1]
    double* d_x = nullptr;        // assess: [B][n]
    double* d_grad = nullptr;     // assess: [B][n]
    double* d_beta = nullptr;     // assess: beta [B], gamma [B]
    double* d_margins = nullptr;  // [B][m], allocated by the first ellhip_batch_svm_margins
    hipStream_t stream = nullptr;
};

namespace {

BatchSvmArrays batch_svm_arrays(ellhip_batch_svm* o) {
    const size_t B = (size_t)o->B;
    BatchSvmArrays A;
    A.XT = o->d_XT;
    A.labels = o->d_labels;
    A.tab_stride = o->shared ? 0 : (long long)o->nfeat * o->ld;
    A.min_idx = o->d_minidx;
    A.min_val = o->d_minval;
    A.gamma = o->d_gamma;
    A.xbest = o->d_xbest;
    A.has_best = o->d_ints;
    A.niter = o->d_niter;
    A.stopped = o->d_ints + B;
    A.status = o->d_ints + 2 * B;
    A.nstopped = o->d_ints + 3 * B;
    return A;
}

// one scan per problem at x; any of the outputs may be null
int batch_svm_assess(ellhip_batch_svm* o, const double* x, int keep_last, double* gamma_out, double* grad_out,
                     double* beta_out, double* margins_out) {
    DeviceGuard guard(o->device);
    const size_t B = (size_t)o->B, n = (size_t)o->n, m = (size_t)o->m;
    if (margins_out && !o->d_margins) {
        const hipError_t e = hipMalloc(&o->d_margins, B * m * sizeof(double));
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched svm margins allocation", e);
    }
    const int T = o->n <= 64 ? 256 : 128;
    const int epw = std::min(64, T / o->n);
    const size_t lds = (size_t)epw * (batch_svm_lds_doubles(o->n) + n) * sizeof(double);  // at most 64 * 15 * 8 bytes
    const unsigned grid = (unsigned)((o->B + epw - 1) / epw);
    BatchSvmArrays A = batch_svm_arrays(o);
    double* d_beta = o->d_beta;
    double* d_gamma = o->d_beta + B;
    HIPCHK(hipMemcpy(o->d_x, x, B * n * sizeof(double), hipMemcpyHostToDevice));
#define BATCH_SVM_ASSESS(TT)                                                                                           \
    hipLaunchKernelGGL(k_batch_svm_assess<TT>, dim3(grid), dim3(TT), lds, o->stream, o->B, o->n, epw, o->m, o->ld,     \
                       keep_last, A, (const double*)o->d_x, d_gamma, o->d_grad, d_beta,                                \
                       margins_out ? o->d_margins : (double*)nullptr)
    if (T == 128) BATCH_SVM_ASSESS(128);
    else BATCH_SVM_ASSESS(256);
#undef BATCH_SVM_ASSESS
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(o->stream));
    if (gamma_out) HIPCHK(hipMemcpy(gamma_out, d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    if (grad_out) HIPCHK(hipMemcpy(grad_out, o->d_grad, B * n * sizeof(double), hipMemcpyDeviceToHost));
    if (beta_out) HIPCHK(hipMemcpy(beta_out, d_beta, B * sizeof(double), hipMemcpyDeviceToHost));
    if (margins_out) HIPCHK(hipMemcpy(margins_out, o->d_margins, B * m * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

int ellhip_batch_svm_create(ellhip_batch_svm** out, int64_t B, int64_t m, int64_t nfeat, const double* data,
                            int32_t shared_data, const int32_t* labels, int device) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1 || B > (1 << 24)) return fail(ELLHIP_E_INVALID, "batched svm: need 1 <= B <= 2^24");
    if (m < 1 || m > (1 << 24)) return fail(ELLHIP_E_INVALID, "batched svm: need 1 <= m <= 2^24 samples");
    if (nfeat < 1 || nfeat > BATCH_NMAX - 1) return fail(ELLHIP_E_INVALID, "batched svm: need 1 <= nfeat <= 127 features");
    if (!data || !labels) return fail(ELLHIP_E_INVALID, "NULL argument");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched svm loop has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_batch_svm* o = new (std::nothrow) ellhip_batch_svm();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->device = device;
    o->B = B;
    o->m = (int)m;
    o->nfeat = (int)nfeat;
    o->n = (int)nfeat + 1;
    o->ld = (m + 7) / 8 * 8;
    o->shared = shared_data != 0;
    DeviceGuard guard(device);
    auto bail = [&](int code) {
        ellhip_batch_svm_destroy(o);
        return code;
    };
    const size_t sB = (size_t)B, sn = (size_t)o->n, sm = (size_t)m, sf = (size_t)nfeat;
    const size_t ntab = o->shared ? 1 : sB;
    const size_t tbytes = ntab * sf * (size_t)o->ld * sizeof(double);
    hipError_t e = hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&o->d_XT, tbytes);
    if (e == hipSuccess) e = hipMalloc(&o->d_labels, sB * sm * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&o->d_minidx, sB * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(&o->d_minval, sB * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_gamma, sB * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_xbest, sB * sn * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_niter, sB * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(&o->d_ints, (3 * sB + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&o->d_x, sB * sn * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_grad, sB * sn * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_beta, 2 * sB * sizeof(double));
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched svm allocation", e));
    // every fill is complete before anything else touches its buffer (fill_now waits)
    if (o->ld != m) e = fill_now(o->d_XT, 0, tbytes, o->stream);  // the padding samples read as 0 and are never used
    if (e == hipSuccess) e = fill_now(o->d_minidx, 0, sB * sizeof(long long), o->stream);
    if (e == hipSuccess) e = fill_now(o->d_gamma, 0, sB * sizeof(double), o->stream);
    if (e == hipSuccess) e = fill_now(o->d_xbest, 0, sB * sn * sizeof(double), o->stream);
    if (e == hipSuccess) e = fill_now(o->d_niter, 0, sB * sizeof(long long), o->stream);
    if (e == hipSuccess) e = fill_now(o->d_ints, 0, (3 * sB + 1) * sizeof(int), o->stream);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched svm memset", e));
    {  // min_val = +inf, min_idx = 0: nothing scanned yet
        std::vector<double> inf(sB, __builtin_inf());
        e = hipMemcpy(o->d_minval, inf.data(), sB * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemcpy(o->d_labels, labels, sB * sm * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched svm labels upload", e));
    // the tables, taken as one [ntab * m][nfeat] matrix: bounded slabs of its rows into one staging buffer, transposed on
    // the device (peak device memory is the tables plus one slab; no host transpose)
    const long long total = (long long)ntab * m;
    const long long slab_rows = std::max<long long>(1, std::min<long long>(total, (64LL << 20) / (nfeat * 8)));
    double* d_slab = nullptr;
    e = hipMalloc(&d_slab, (size_t)slab_rows * sf * sizeof(double));
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched svm staging allocation", e));
    for (long long r0 = 0; r0 < total && e == hipSuccess; r0 += slab_rows) {
        const long long rows = std::min(total - r0, slab_rows);
        e = hipMemcpyAsync(d_slab, data + (size_t)r0 * sf, (size_t)rows * sf * sizeof(double), hipMemcpyHostToDevice,
                           o->stream);
        if (e != hipSuccess) break;
        const long long tiles = ((nfeat + BATCH_SVM_TILE - 1) / BATCH_SVM_TILE) * ((rows + BATCH_SVM_TILE - 1) / BATCH_SVM_TILE);
        hipLaunchKernelGGL(k_batch_svm_transpose, dim3((unsigned)std::min<long long>(tiles, 4096)), dim3(256), 0, o->stream,
                           (const double*)d_slab, rows, r0, (long long)m, (long long)nfeat, o->ld, o->d_XT);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(o->stream);  // the slab is overwritten next
    }
    (void)hipFree(d_slab);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched svm table upload", e));
    *out = o;
    return 0;
}

void ellhip_batch_svm_destroy(ellhip_batch_svm* o) {
    if (!o) return;
    DeviceGuard guard(o->device);
    if (o->stream) (void)hipStreamSynchronize(o->stream);
    void* bufs[] = {o->d_XT,    o->d_labels, o->d_minidx, o->d_minval, o->d_gamma, o->d_xbest,
                    o->d_niter, o->d_ints,   o->d_x,      o->d_grad,   o->d_beta,  o->d_margins};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    if (o->stream) (void)hipStreamDestroy(o->stream);
    delete o;
}

int ellhip_batch_svm_margins(ellhip_batch_svm* o, const double* x, double* margins_out) {
    if (!o || !x || !margins_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_svm_assess(o, x, 0, nullptr, nullptr, nullptr, margins_out);
}

int ellhip_batch_svm_assess_optim(ellhip_batch_svm* o, const double* x, double* gamma_out, double* grad_out,
                                  double* beta_out) {
    if (!o || !x || !gamma_out || !grad_out || !beta_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_svm_assess(o, x, 1, gamma_out, grad_out, beta_out, nullptr);
}

int ellhip_batch_svm_last(ellhip_batch_svm* o, int64_t* min_idx, double* min_val) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(o->device);
    HIPCHK(hipStreamSynchronize(o->stream));
    const size_t B = (size_t)o->B;
    if (min_idx) {
        std::vector<long long> idx(B);
        HIPCHK(hipMemcpy(idx.data(), o->d_minidx, B * sizeof(long long), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) min_idx[b] = idx[b];
    }
    if (min_val) HIPCHK(hipMemcpy(min_val, o->d_minval, B * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// stable: the spaces are EllStable (include/ellhip_batch_stable_loops.h)
static int batch_svm_run(ellhip_batch* s, ellhip_batch_svm* o, double* gamma_inout, int64_t max_iters, double tol,
                         double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out, bool stable) {
    if (!s || !o || !gamma_inout || !has_best_out || !niter_out || !status_out)
        return fail(ELLHIP_E_INVALID, "NULL argument");
    if (const int rc = batch_loop_check(s, stable, "batched svm loop")) return rc;
    if (s->B != o->B || s->n != o->n)
        return fail(ELLHIP_E_INVALID, "batched svm loop: spaces and oracle differ in B or n (n = nfeat + 1)");
    if (s->device != o->device)
        return fail(ELLHIP_E_INVALID, "batched svm loop: spaces and oracle live on different devices");
    if (max_iters < 0) return fail(ELLHIP_E_INVALID, "max_iters must be >= 0");
    const size_t B = (size_t)o->B, n = (size_t)o->n;
    const BatchLoopShape sh = batch_loop_shape(s, stable);
    const size_t lds = (size_t)sh.epw * (sh.space_doubles + batch_svm_lds_doubles(s->n)) * sizeof(double);
    if (lds > BATCH_LMI_LDS_MAX) return fail(ELLHIP_E_INVALID, "batched svm loop: this n needs more LDS than a workgroup has");
    DeviceGuard guard(s->device);
    BatchSvmArrays A = batch_svm_arrays(o);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
    HIPCHK(fill_now(o->d_ints, 0, (3 * B + 1) * sizeof(int), s->stream));
    HIPCHK(fill_now(o->d_niter, 0, B * sizeof(long long), s->stream));
    HIPCHK(hipMemcpy(o->d_gamma, gamma_inout, B * sizeof(double), hipMemcpyHostToDevice));
    const BatchParams P = batch_loop_params(s, sh);
    const unsigned grid = (unsigned)((s->B + sh.epw - 1) / sh.epw);
    const EllCalcDev calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    BatchSvmLoop R;
    R.m = o->m;
    R.ld = o->ld;
    R.max_iters = max_iters;
    R.tol = tol;
    for (long long done = 0; done < max_iters; done += o->chunk) {
        R.iters = (int)std::min<long long>(o->chunk, max_iters - done);
#define BATCH_SVM_GO(TT, ST)                                                                                          \
    do {                                                                                                              \
        const int rc_ = batch_lmi_allow_lds(&k_batch_svm_loop<TT, ST>, s->device, sh.slot, lds);                      \
        if (rc_) return rc_;                                                                                          \
        hipLaunchKernelGGL((k_batch_svm_loop<TT, ST>), dim3(grid), dim3(TT), lds, s->stream, P, R, s->d_Q, s->d_xc,   \
                           s->d_kappa, s->d_tsq, A, calc);                                                            \
    } while (0)
        if (stable) {
            if (sh.T == 128) BATCH_SVM_GO(128, true);
            else BATCH_SVM_GO(256, true);
        } else if (sh.T == 64) BATCH_SVM_GO(64, false);
        else if (sh.T == 128) BATCH_SVM_GO(128, false);
        else BATCH_SVM_GO(256, false);
#undef BATCH_SVM_GO
        HIPCHK(hipGetLastError());
        int nstopped = 0;
        HIPCHK(hipMemcpyAsync(&nstopped, A.nstopped, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        if ((long long)nstopped >= o->B) break;
    }
    std::vector<int32_t> has(B);
    std::vector<long long> niter(B);
    HIPCHK(hipMemcpy(has.data(), A.has_best, B * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status_out, A.status, B * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(niter.data(), o->d_niter, B * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(gamma_inout, o->d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        has_best_out[b] = has[b];
        niter_out[b] = niter[b];
    }
    if (x_best_out) {
        std::vector<double> xb(B * n);
        HIPCHK(hipMemcpy(xb.data(), o->d_xbest, B * n * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b)
            if (has[b]) memcpy(x_best_out + b * n, xb.data() + b * n, n * sizeof(double));
    }
    return 0;
}

int ellhip_batch_svm_optim(ellhip_batch* s, ellhip_batch_svm* o, double* gamma_inout, int64_t max_iters, double tol,
                           double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out) {
    return batch_svm_run(s, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out, false);
}

int ellhip_batch_svm_set_chunk(ellhip_batch_svm* o, int64_t iters) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (iters < 1 || iters > 4096) return fail(ELLHIP_E_INVALID, "batched svm: chunk must be in 1..4096");
    o->chunk = (int)iters;
    return 0;
}

}  // extern "C"
