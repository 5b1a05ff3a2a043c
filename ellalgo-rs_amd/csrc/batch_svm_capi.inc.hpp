// batch_svm_capi.inc.hpp -- C ABI of the batched device-resident SVM cutting-plane loop (include/ellhip_batch_svm.h).
// Included at the end of ellhip_capi.hip, after batch_loop_capi.inc.hpp (the loop state, the launch shapes and the driver).
//
// Reference: src/oracles/svm_oracle.rs:4-58 (oracle), src/cutting_plane.rs:286-313 (loop).
#include "../../include/ellhip_batch_svm.h"

#include "batch_svm_kernels.hpp"

struct ellhip_batch_svm {
    BatchLoopBuffers loop;        // device, B, n, stream, the loop state
    long long B = 0;
    int m = 0;
    int nfeat = 0;
    int n = 0;                    // nfeat + 1
    long long ld = 0;             // m rounded up to 8 doubles
    int shared = 0;
    double* d_XT = nullptr;       // [ntab][nfeat][ld], ntab = 1 (shared) or B
    int* d_labels = nullptr;      // [B][m]
    long long* d_minidx = nullptr;  // [B]
    double* d_minval = nullptr;   // [B]
    double* d_x = nullptr;        // assess: [B][n]
    double* d_grad = nullptr;     // assess: [B][n]
    double* d_beta = nullptr;     // assess: beta [B], gamma [B]
    double* d_margins = nullptr;  // [B][m], allocated by the first ellhip_batch_svm_margins
};

namespace {

BatchSvmOracle::Args batch_svm_args(const ellhip_batch_svm* o) {
    BatchSvmOracle::Args A;
    A.XT = o->d_XT;
    A.labels = o->d_labels;
    A.tab_stride = o->shared ? 0 : (long long)o->nfeat * o->ld;
    A.min_idx = o->d_minidx;
    A.min_val = o->d_minval;
    A.m = o->m;
    A.ld = o->ld;
    return A;
}

// one scan per problem at x; any of the outputs may be null
int batch_svm_assess(ellhip_batch_svm* o, const double* x, int keep_last, double* gamma_out, double* grad_out,
                     double* beta_out, double* margins_out) {
    DeviceGuard guard(o->loop.device);
    const size_t B = (size_t)o->B, n = (size_t)o->n, m = (size_t)o->m;
    if (margins_out && !o->d_margins) {
        const hipError_t e = o->loop.mem.device(o->d_margins, B * m * sizeof(double));
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched svm margins allocation", e);
    }
    const size_t per = batch_svm_lds_doubles(o->n) + n;
    // past the LDS engine's n (batch_row_shape has no instance per workgroup to offer): one instance per workgroup, n threads
    // rounded up to whole waves, as the streamed engine shapes its own
    const bool wide = o->n > BATCH_NMAX;
    const BatchRowShape sh = batch_row_shape(o->n, per);
    const int T = wide ? (o->n + 63) / 64 * 64 : sh.T, epw = wide ? 1 : sh.epw;
    const size_t lds = (size_t)epw * per * sizeof(double);  // at most 64 * 15 * 8 bytes, or 16.1 KiB at n = 1024
    const unsigned grid = (unsigned)((o->B + epw - 1) / epw);
    const BatchSvmOracle::Args A = batch_svm_args(o);
    double* d_beta = o->d_beta;
    double* d_gamma = o->d_beta + B;
    HIPCHK(hipMemcpy(o->d_x, x, B * n * sizeof(double), hipMemcpyHostToDevice));
#define BATCH_SVM_ASSESS(TT)                                                                                           \
    hipLaunchKernelGGL(k_batch_svm_assess<TT>, dim3(grid), dim3(T), lds, o->loop.stream, o->B, o->n, epw, keep_last,   \
                       A, (const double*)o->d_x, d_gamma, o->d_grad, d_beta,                                           \
                       margins_out ? o->d_margins : (double*)nullptr)
    if (wide) BATCH_SVM_ASSESS(1024);  // (the template argument bounds the block; the block is T threads)
    else if (T == 128) BATCH_SVM_ASSESS(128);
    else BATCH_SVM_ASSESS(256);
#undef BATCH_SVM_ASSESS
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    if (gamma_out) HIPCHK(hipMemcpy(gamma_out, d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    if (grad_out) HIPCHK(hipMemcpy(grad_out, o->d_grad, B * n * sizeof(double), hipMemcpyDeviceToHost));
    if (beta_out) HIPCHK(hipMemcpy(beta_out, d_beta, B * sizeof(double), hipMemcpyDeviceToHost));
    if (margins_out) HIPCHK(hipMemcpy(margins_out, o->d_margins, B * m * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// nfeat_max: 127 for the LDS engine's constructor, 1023 for the streamed one (batch_svm_streamed_capi.inc.hpp)
int batch_svm_create(ellhip_batch_svm** out, int64_t B, int64_t m, int64_t nfeat, const double* data, int32_t shared_data,
                     const int32_t* labels, int device, int nfeat_max) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1 || B > (1 << 24)) return fail(ELLHIP_E_INVALID, "batched svm: need 1 <= B <= 2^24");
    if (m < 1 || m > (1 << 24)) return fail(ELLHIP_E_INVALID, "batched svm: need 1 <= m <= 2^24 samples");
    if (nfeat < 1 || nfeat > nfeat_max)
        return fail(ELLHIP_E_INVALID, ("batched svm: need 1 <= nfeat <= " + std::to_string(nfeat_max) + " features").c_str());
    if (!data || !labels) return fail(ELLHIP_E_INVALID, "NULL argument");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched svm loop has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_batch_svm* o = new (std::nothrow) ellhip_batch_svm();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
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
    hipError_t e = batch_loop_alloc(o->loop, device, B, o->n);
    if (e == hipSuccess) e = o->loop.mem.device(o->d_XT, tbytes);
    if (e == hipSuccess) e = o->loop.mem.device(o->d_labels, sB * sm * sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_minidx, sB * sizeof(long long));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_minval, sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_x, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_grad, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_beta, 2 * sB * sizeof(double));
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched svm allocation", e));
    // every fill is complete before anything else touches its buffer (fill_now waits)
    if (o->ld != m) e = fill_now(o->d_XT, 0, tbytes, o->loop.stream);  // the padding samples read as 0 and are never used
    if (e == hipSuccess) e = fill_now(o->d_minidx, 0, sB * sizeof(long long), o->loop.stream);
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
    Allocs slab;  // (gone on every return path)
    double* d_slab = nullptr;
    e = slab.device(d_slab, (size_t)slab_rows * sf * sizeof(double));
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched svm staging allocation", e));
    for (long long r0 = 0; r0 < total && e == hipSuccess; r0 += slab_rows) {
        const long long rows = std::min(total - r0, slab_rows);
        e = hipMemcpyAsync(d_slab, data + (size_t)r0 * sf, (size_t)rows * sf * sizeof(double), hipMemcpyHostToDevice,
                           o->loop.stream);
        if (e != hipSuccess) break;
        const long long tiles = ((nfeat + BATCH_SVM_TILE - 1) / BATCH_SVM_TILE) * ((rows + BATCH_SVM_TILE - 1) / BATCH_SVM_TILE);
        hipLaunchKernelGGL(k_batch_svm_transpose, dim3((unsigned)std::min<long long>(tiles, 4096)), dim3(256), 0, o->loop.stream,
                           (const double*)d_slab, rows, r0, (long long)m, (long long)nfeat, o->ld, o->d_XT);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(o->loop.stream);  // the slab is overwritten next
    }
    slab.release_all();
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched svm table upload", e));
    *out = o;
    return 0;
}

}  // namespace

extern "C" {

int ellhip_batch_svm_create(ellhip_batch_svm** out, int64_t B, int64_t m, int64_t nfeat, const double* data,
                            int32_t shared_data, const int32_t* labels, int device) {
    return batch_svm_create(out, B, m, nfeat, data, shared_data, labels, device, BATCH_NMAX - 1);
}

void ellhip_batch_svm_destroy(ellhip_batch_svm* o) {
    if (!o) return;
    DeviceGuard guard(o->loop.device);
    batch_loop_free(o->loop);
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
    DeviceGuard guard(o->loop.device);
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    const size_t B = (size_t)o->B;
    if (min_idx) {
        std::vector<long long> idx(B);
        HIPCHK(hipMemcpy(idx.data(), o->d_minidx, B * sizeof(long long), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) min_idx[b] = idx[b];
    }
    if (min_val) HIPCHK(hipMemcpy(min_val, o->d_minval, B * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// the loop of all three headers (ellhip_batch_svm.h, ellhip_batch_stable_loops.h, ellhip_batch_svm_streamed.h) on `engine`
static int batch_svm_run(ellhip_batch* s, ellhip_batch_svm* o, double* gamma_inout, int64_t max_iters, double tol,
                         double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out,
                         BatchLoopEngine engine) {
    if (!s || !o || !gamma_inout || !has_best_out || !niter_out || !status_out)
        return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_loop_run<BatchSvmOracle>(s, o->loop, batch_svm_args(o), {"svm", "n", " (n = nfeat + 1)"}, engine, 0,
                                          gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out);
}

int ellhip_batch_svm_optim(ellhip_batch* s, ellhip_batch_svm* o, double* gamma_inout, int64_t max_iters, double tol,
                           double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out) {
    return batch_svm_run(s, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out, BATCH_ENGINE_LDS);
}

int ellhip_batch_svm_set_chunk(ellhip_batch_svm* o, int64_t iters) {
    return batch_loop_set_chunk(o ? &o->loop : nullptr, iters, "batched svm");
}

}  // extern "C"
