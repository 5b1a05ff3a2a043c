// svm_capi.inc.hpp -- C ABI of the device-side SvmOracle and of the device-resident cutting-plane loop built on it.
// Included at the end of ellhip_capi.hip (same translation unit: the loop issues the primitives of ell_primitives_capi.inc.hpp directly).
//
// Reference: src/oracles/svm_oracle.rs:4-58 (oracle), src/cutting_plane.rs:286-313 (loop).
#include "../../include/ellhip_svm.h"

#include "svm_kernels.hpp"
#include "device_loop.inc.hpp"

struct ellhip_svm {
    int device = 0;
    SvmParams P{};
    bool nt = false;
    unsigned grid = 1;
    Allocs mem;
    double* d_XT = nullptr;     // nfeat x ld, feature-major
    int* d_labels = nullptr;    // m
    SvmPartial* d_part = nullptr;  // grid
    double* d_x = nullptr;      // nfeat + 1
    double* d_g = nullptr;      // nfeat + 1
    double* d_xbest = nullptr;  // nfeat + 1
    double* d_margins = nullptr;  // m, allocated by the first ellhip_svm_margins
    SvmState* d_ss = nullptr;
    CutParams* d_cp = nullptr;
    int* d_zero = nullptr;
    hipStream_t stream = nullptr;
    SvmState* h_ss = nullptr;
    CutParams* h_cp = nullptr;
    double* h_vec = nullptr;    // nfeat + 1
};

namespace {

// one scan: margins (into `margins` when given) and the per-workgroup argmin, then the cut (xbest: device loop)
int svm_issue(ellhip_svm* o, hipStream_t st, const double* x_dev, double* margins, double* xbest, const int* halted) {
    if (o->nt)
        hipLaunchKernelGGL(k_svm_margins<true>, dim3(o->grid), dim3(SVM_THREADS), 0, st, (const double*)o->d_XT,
                           (const int*)o->d_labels, o->P, x_dev, margins, o->d_part, halted);
    else
        hipLaunchKernelGGL(k_svm_margins<false>, dim3(o->grid), dim3(SVM_THREADS), 0, st, (const double*)o->d_XT,
                           (const int*)o->d_labels, o->P, x_dev, margins, o->d_part, halted);
    hipLaunchKernelGGL(k_svm_final, dim3(1), dim3(SVM_THREADS), 0, st, (const double*)o->d_XT, (const int*)o->d_labels,
                       o->P, (const SvmPartial*)o->d_part, (long long)o->grid, x_dev, o->d_ss, o->d_g, o->d_cp, xbest,
                       halted);
    HIPCHK(hipGetLastError());
    return 0;
}

int svm_upload_x(ellhip_svm* o, const double* x) {
    const size_t vbytes = (size_t)(o->P.nfeat + 1) * sizeof(double);
    memcpy(o->h_vec, x, vbytes);
    HIPCHK(hipMemcpyAsync(o->d_x, o->h_vec, vbytes, hipMemcpyHostToDevice, o->stream));
    return 0;
}

// The oracle's side of the device-resident loop (device_loop.inc.hpp): cutting_plane_optim (src/cutting_plane.rs:286-313).
// assess_optim always answers shrunk = true, so k_svm_final records x_best = xc and asks for a central cut every time.
struct SvmStage {
    ellhip_svm* o;
    double* gamma_inout;
    double* x_best_out;
    int* has_best_out;
    int64_t* niter_out;

    hipStream_t stream() { return o->stream; }
    const double* grad() { return o->d_g; }
    const CutParams* cut() { return o->d_cp; }
    int begin(hipStream_t st) {
        SvmState ss;
        memset(&ss, 0, sizeof ss);
        ss.min_val = __builtin_inf();
        ss.gamma = *gamma_inout;  // unchanged when the loop runs no iteration
        *o->h_ss = ss;
        HIPCHK(hipMemcpyAsync(o->d_ss, o->h_ss, sizeof(SvmState), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    int issue(hipStream_t st, ellhip_space* s, const int* halted) {
        return svm_issue(o, st, s->d_xc, nullptr, o->d_xbest, halted);
    }
    int finish(hipStream_t st, long long niter) {
        HIPCHK(hipMemcpyAsync(o->h_ss, o->d_ss, sizeof(SvmState), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *niter_out = niter;
        *has_best_out = o->h_ss->has_best;
        if (o->h_ss->has_best && x_best_out) {
            const size_t vbytes = (size_t)(o->P.nfeat + 1) * sizeof(double);
            HIPCHK(hipMemcpyAsync(o->h_vec, o->d_xbest, vbytes, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            memcpy(x_best_out, o->h_vec, vbytes);
        }
        *gamma_inout = o->h_ss->gamma;
        return 0;
    }
};

}  // namespace

extern "C" {

int ellhip_svm_create(ellhip_svm** out, int64_t m, int64_t nfeat, const double* data, const int32_t* labels, int device) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (m < 1 || nfeat < 1) return fail(ELLHIP_E_INVALID, "svm oracle needs m >= 1 samples and nfeat >= 1 features");
    if (m > (1LL << 33) || nfeat > (1LL << 33)) return fail(ELLHIP_E_INVALID, "svm oracle: more than 2^33 samples or features");
    if (!data || !labels) return fail(ELLHIP_E_INVALID, "NULL argument");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the svm oracle has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_svm* o = new (std::nothrow) ellhip_svm();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->device = device;
    o->P.m = m;
    o->P.nfeat = nfeat;
    o->P.ld = (m + SVM_LD_ALIGN - 1) / SVM_LD_ALIGN * SVM_LD_ALIGN;
    const double t_bytes = (double)nfeat * (double)o->P.ld * 8.0;
    o->nt = t_bytes > 200.0 * 1024 * 1024;  // same rule as the Q stream: larger than the Infinity Cache share
    o->grid = (unsigned)((m + SVM_SPW - 1) / SVM_SPW);
    DeviceGuard guard(device);
    auto bail = [&](int code) {
        ellhip_svm_destroy(o);
        return code;
    };
    const long long n = nfeat + 1;
    const size_t vbytes = (size_t)n * sizeof(double);
    const size_t tbytes = (size_t)nfeat * (size_t)o->P.ld * sizeof(double);
    hipError_t e = hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = o->mem.device(o->d_XT, tbytes);
    if (e == hipSuccess) e = o->mem.device(o->d_labels, (size_t)m * sizeof(int));
    if (e == hipSuccess) e = o->mem.device(o->d_part, (size_t)o->grid * sizeof(SvmPartial));
    if (e == hipSuccess) e = o->mem.device(o->d_x, vbytes);
    if (e == hipSuccess) e = o->mem.device(o->d_g, vbytes);
    if (e == hipSuccess) e = o->mem.device(o->d_xbest, vbytes);
    if (e == hipSuccess) e = o->mem.device(o->d_ss, sizeof(SvmState));
    if (e == hipSuccess) e = o->mem.device(o->d_cp, sizeof(CutParams));
    if (e == hipSuccess) e = o->mem.device(o->d_zero, sizeof(int));
    if (e == hipSuccess) e = o->mem.pinned(o->h_ss, sizeof(SvmState), hipHostMallocDefault);
    if (e == hipSuccess) e = o->mem.pinned(o->h_cp, sizeof(CutParams), hipHostMallocDefault);
    if (e == hipSuccess) e = o->mem.pinned(o->h_vec, vbytes, hipHostMallocDefault);
    if (e != hipSuccess) return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "svm allocation", e));
    if (o->P.ld != m) e = fill_now(o->d_XT, 0, tbytes, o->stream);  // the padding samples read as 0 and are never used
    if (e == hipSuccess) e = fill_now(o->d_zero, 0, sizeof(int), o->stream);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "svm memset", e));
    e = hipMemcpy(o->d_labels, labels, (size_t)m * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "svm labels upload", e));
    // the table: bounded slabs of the caller's rows into one staging buffer, transposed on the device (peak device
    // memory is the table plus one slab; no host transpose)
    const long long slab_rows = std::max<long long>(1, std::min<long long>(m, (64LL << 20) / (nfeat * 8)));
    Allocs slab;  // (gone on every return path)
    double* d_slab = nullptr;
    e = slab.device(d_slab, (size_t)slab_rows * (size_t)nfeat * sizeof(double));
    if (e != hipSuccess) return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "svm staging allocation", e));
    for (long long r0 = 0; r0 < m && e == hipSuccess; r0 += slab_rows) {
        const long long rows = std::min(m - r0, slab_rows);
        e = hipMemcpyAsync(d_slab, data + (size_t)r0 * (size_t)nfeat, (size_t)rows * (size_t)nfeat * sizeof(double),
                           hipMemcpyHostToDevice, o->stream);
        if (e != hipSuccess) break;
        const long long tiles = ((nfeat + SVM_TILE - 1) / SVM_TILE) * ((rows + SVM_TILE - 1) / SVM_TILE);
        hipLaunchKernelGGL(k_svm_transpose, dim3((unsigned)std::min<long long>(tiles, 4096)), dim3(256), 0, o->stream,
                           (const double*)d_slab, rows, r0, o->P, o->d_XT);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(o->stream);  // the slab is overwritten next
    }
    slab.release_all();
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "svm table upload", e));
    SvmState ss;
    memset(&ss, 0, sizeof ss);
    ss.min_val = __builtin_inf();
    *o->h_ss = ss;
    e = hipMemcpy(o->d_ss, o->h_ss, sizeof(SvmState), hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "svm state upload", e));
    *out = o;
    return 0;
}

void ellhip_svm_destroy(ellhip_svm* o) {
    if (!o) return;
    DeviceGuard guard(o->device);
    if (o->stream) (void)hipStreamSynchronize(o->stream);
    o->mem.release_all();
    if (o->stream) (void)hipStreamDestroy(o->stream);
    delete o;
}

int ellhip_svm_assess_optim(ellhip_svm* o, const double* x, double* gamma_inout, double* grad_out, double* beta_out,
                            int* shrunk_out) {
    if (!o || !x || !gamma_inout || !grad_out || !beta_out || !shrunk_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->device);
    int rc = svm_upload_x(o, x);
    if (rc) return rc;
    rc = svm_issue(o, o->stream, o->d_x, nullptr, nullptr, o->d_zero);
    if (rc) return rc;
    const size_t vbytes = (size_t)(o->P.nfeat + 1) * sizeof(double);
    HIPCHK(hipMemcpyAsync(o->h_ss, o->d_ss, sizeof(SvmState), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(hipMemcpyAsync(o->h_cp, o->d_cp, sizeof(CutParams), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(hipMemcpyAsync(o->h_vec, o->d_g, vbytes, hipMemcpyDeviceToHost, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
    memcpy(grad_out, o->h_vec, vbytes);
    *beta_out = o->h_cp->b0;
    *gamma_inout = o->h_ss->gamma;
    *shrunk_out = 1;
    return 1;
}

int ellhip_svm_margins(ellhip_svm* o, const double* x, double* margins_out) {
    if (!o || !x || !margins_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->device);
    const size_t mbytes = (size_t)o->P.m * sizeof(double);
    if (!o->d_margins) {
        const hipError_t e = o->mem.device(o->d_margins, mbytes);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "svm margins allocation", e);
    }
    int rc = svm_upload_x(o, x);
    if (rc) return rc;
    rc = svm_issue(o, o->stream, o->d_x, o->d_margins, nullptr, o->d_zero);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(margins_out, o->d_margins, mbytes, hipMemcpyDeviceToHost, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
    return 0;
}

int ellhip_svm_last(ellhip_svm* o, int64_t* min_idx, double* min_val) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(o->device);
    HIPCHK(hipStreamSynchronize(o->stream));
    HIPCHK(hipMemcpy(o->h_ss, o->d_ss, sizeof(SvmState), hipMemcpyDeviceToHost));
    if (min_idx) *min_idx = o->h_ss->min_idx;
    if (min_val) *min_val = o->h_ss->min_val;
    return 0;
}

int ellhip_svm_optim(ellhip_space* s, ellhip_svm* o, double* gamma_inout, int64_t max_iters, double tol,
                     double* x_best_out, int* has_best_out, int64_t* niter_out) {
    if (!s || !o || !gamma_inout || !has_best_out || !niter_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    SvmStage stage{o, gamma_inout, x_best_out, has_best_out, niter_out};
    return drive_device_loop(s, stage, o->P.nfeat + 1, o->device, max_iters, tol);
}

}  // extern "C"
