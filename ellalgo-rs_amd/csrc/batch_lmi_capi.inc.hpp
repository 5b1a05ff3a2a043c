// batch_lmi_capi.inc.hpp -- C ABI of the batched device-resident LMI cutting-plane loop (include/ellhip_batch_lmi.h).
// Included at the end of ellhip_capi.hip, after batch_capi.inc.hpp (it drives the batch engine's handle directly).
//
// Reference: tests/lmi_tests.rs:142-171 (oracle), src/oracles/lmi_oracle.rs, lmi0_oracle.rs, ldlt_mgr.rs,
// src/cutting_plane.rs:205-227, 286-313 (loops).
#include "../../include/ellhip_batch_lmi.h"

#include "batch_lmi_kernels.hpp"

struct ellhip_batch_lmi {
    int device = 0;
    long long B = 0;
    int n = 0;
    BatchLmiParams L{};
    int chunk = 256;
    double* d_pencil = nullptr;   // [B][block][a][b][k]
    double* d_matb = nullptr;     // [B][block][a][b], or null
    double* d_c = nullptr;        // [B][n], or null
    int* d_idx = nullptr;         // [B]
    double* d_gamma = nullptr;    // [B]
    double* d_xbest = nullptr;    // [B][n]
    long long* d_niter = nullptr; // [B]
    int* d_ints = nullptr;        // has_best [B], stopped [B], status [B], nstopped [1]
    double* d_x = nullptr;        // assess: [B][n]
    double* d_grad = nullptr;     // assess: [B][n]
    double* d_beta = nullptr;     // assess: [B]
    hipStream_t stream = nullptr;
};

namespace {

// 160 KiB per workgroup, less the 1 KiB kept for the kernel's static LDS (the barrier votes)
constexpr size_t BATCH_LMI_LDS_MAX = 159 * 1024;

// more than the default 64 KiB of dynamic LDS needs an opt-in per kernel and per device; as in batch_shape it is only ever
// raised, with the high-water marks kept per (device, block size)
template <class K>
int batch_lmi_allow_lds(K kernel, int device, int slot, size_t bytes) {
    constexpr int MAXDEV = 64;
    static std::atomic<int> granted[MAXDEV][6];  // T = 64, 128, 256 on Ell, then on EllStable
    const bool known = device >= 0 && device < MAXDEV;
    if (known && (int)bytes <= granted[device][slot].load()) return 0;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (known) {
        int seen = granted[device][slot].load();
        while (seen < (int)bytes && !granted[device][slot].compare_exchange_weak(seen, (int)bytes)) {}
    }
    return 0;
}

// How a loop kernel is launched on a batch handle.  An Ell handle is launched as the batch engine shaped it.  An EllStable
// handle is shaped for k_batch_update_stable's one lane per ellipsoid (one wave, up to 64 ellipsoids); the loop kernels
// give an instance n threads, so they take the Ell rule for T and epw with batch_stable_apply_lds_doubles in it.  slot:
// the entry of batch_lmi_allow_lds's table (the Ell and EllStable instantiations of a kernel have the same type).
struct BatchLoopShape {
    int T = 64, epw = 1, slot = 0;
    size_t space_doubles = 0;  // LDS doubles of one instance's space
};

BatchLoopShape batch_loop_shape(const ellhip_batch* s, bool stable) {
    BatchLoopShape sh;
    if (!stable) {
        sh.T = s->T;
        sh.epw = s->epw;
        sh.space_doubles = batch_lds_doubles(s->n);
    } else {
        sh.T = s->n <= 64 ? 256 : 128;
        sh.epw = std::min(64, sh.T / s->n);
        sh.space_doubles = batch_stable_apply_lds_doubles(s->n);
        while (sh.epw > 1 && (size_t)sh.epw * sh.space_doubles * sizeof(double) > 64 * 1024) sh.epw -= 1;
    }
    sh.slot = (sh.T == 64 ? 0 : (sh.T == 128 ? 1 : 2)) + (stable ? 3 : 0);
    return sh;
}

// the handle's variant against the entry point's: the plain entry points take Ell handles, the _stable ones EllStable
int batch_loop_check(const ellhip_batch* s, bool stable, const char* what) {
    const int want = stable ? ELLHIP_SPACE_ELL_STABLE : ELLHIP_SPACE_ELL;
    if (s->streamed)  // the loops' kernels keep the matrix in LDS (include/ellhip_batch_streamed.h)
        return fail(ELLHIP_E_INVALID, (std::string(what) + ": streamed batch handles are not supported").c_str());
    if (s->variant == want) return 0;
    const std::string msg = std::string(what) + (stable ? ": the _stable entry points take EllStable batch handles only"
                                                        : ": EllStable batch handles are not supported");
    return fail(ELLHIP_E_INVALID, msg.c_str());
}

BatchParams batch_loop_params(const ellhip_batch* s, const BatchLoopShape& sh) {
    BatchParams P;
    P.B = s->B;
    P.n = s->n;
    P.pitch = batch_pitch(s->n);
    P.epw = sh.epw;
    P.K = 0;
    P.no_defer_trick = s->no_defer_trick;
    return P;
}

// stable: the spaces are EllStable (include/ellhip_batch_stable_loops.h)
int batch_lmi_run(ellhip_batch* s, ellhip_batch_lmi* o, int feas, double* gamma_inout, int64_t max_iters, double tol,
                  double* x_out, int32_t* has_out, int64_t* niter_out, int32_t* status_out, bool stable = false) {
    if (!s || !o || !has_out || !niter_out || !status_out || (!feas && !gamma_inout))
        return fail(ELLHIP_E_INVALID, "NULL argument");
    if (const int rc = batch_loop_check(s, stable, "batched LMI loop")) return rc;
    if (s->B != o->B || s->n != o->n) return fail(ELLHIP_E_INVALID, "batched LMI loop: spaces and oracle differ in B or n");
    if (s->device != o->device) return fail(ELLHIP_E_INVALID, "batched LMI loop: spaces and oracle live on different devices");
    if (!feas && !o->L.has_c) return fail(ELLHIP_E_INVALID, "batched LMI loop: optim needs a handle made with c");
    if (feas && o->L.has_c) return fail(ELLHIP_E_INVALID, "batched LMI loop: feas needs a handle made without c");
    if (max_iters < 0) return fail(ELLHIP_E_INVALID, "max_iters must be >= 0");
    const size_t B = (size_t)o->B, n = (size_t)o->n;
    const BatchLoopShape sh = batch_loop_shape(s, stable);
    const size_t lds = (size_t)sh.epw * (sh.space_doubles + batch_lmi_lds_doubles(s->n, o->L.mmax)) * sizeof(double);
    if (lds > BATCH_LMI_LDS_MAX) return fail(ELLHIP_E_INVALID, "batched LMI loop: this (n, m) needs more LDS than a workgroup has");
    DeviceGuard guard(s->device);
    int* d_has = o->d_ints;
    int* d_stopped = o->d_ints + B;
    int* d_status = o->d_ints + 2 * B;
    int* d_nstopped = o->d_ints + 3 * B;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(fill_now(o->d_ints, 0, (3 * B + 1) * sizeof(int), s->stream));
    HIPCHK(fill_now(o->d_niter, 0, B * sizeof(long long), s->stream));
    if (!feas) HIPCHK(hipMemcpy(o->d_gamma, gamma_inout, B * sizeof(double), hipMemcpyHostToDevice));
    const BatchParams P = batch_loop_params(s, sh);
    const unsigned grid = (unsigned)((s->B + sh.epw - 1) / sh.epw);
    const EllCalcDev calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    BatchLmiLoop R;
    R.feas = feas;
    R.max_iters = max_iters;
    R.tol = tol;
    for (long long done = 0; done < max_iters; done += o->chunk) {
        R.iters = (int)std::min<long long>(o->chunk, max_iters - done);
#define BATCH_LMI_GO(TT, ST)                                                                                           \
    do {                                                                                                                \
        const int rc_ = batch_lmi_allow_lds(&k_batch_lmi_loop<TT, ST>, s->device, sh.slot, lds);                        \
        if (rc_) return rc_;                                                                                            \
        hipLaunchKernelGGL((k_batch_lmi_loop<TT, ST>), dim3(grid), dim3(TT), lds, s->stream, P, o->L, R, s->d_Q,        \
                           s->d_xc, s->d_kappa, s->d_tsq, (const double*)o->d_pencil, (const double*)o->d_matb,         \
                           (const double*)o->d_c, o->d_idx, o->d_gamma, o->d_xbest, d_has, o->d_niter, d_stopped,       \
                           d_status, d_nstopped, calc);                                                                 \
    } while (0)
        if (stable) {
            if (sh.T == 128) BATCH_LMI_GO(128, true);
            else BATCH_LMI_GO(256, true);
        } else if (sh.T == 64) BATCH_LMI_GO(64, false);
        else if (sh.T == 128) BATCH_LMI_GO(128, false);
        else BATCH_LMI_GO(256, false);
#undef BATCH_LMI_GO
        HIPCHK(hipGetLastError());
        int nstopped = 0;
        HIPCHK(hipMemcpyAsync(&nstopped, d_nstopped, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        if ((long long)nstopped >= o->B) break;
    }
    std::vector<int32_t> has(B);
    std::vector<long long> niter(B);
    HIPCHK(hipMemcpy(has.data(), d_has, B * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status_out, d_status, B * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(niter.data(), o->d_niter, B * sizeof(long long), hipMemcpyDeviceToHost));
    if (!feas) HIPCHK(hipMemcpy(gamma_inout, o->d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        has_out[b] = has[b];
        niter_out[b] = niter[b];
    }
    if (x_out) {
        std::vector<double> xb(B * n);
        HIPCHK(hipMemcpy(xb.data(), o->d_xbest, B * n * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b)
            if (has[b]) memcpy(x_out + b * n, xb.data() + b * n, n * sizeof(double));
    }
    return 0;
}

}  // namespace

extern "C" {

int ellhip_batch_lmi_create(ellhip_batch_lmi** out, int64_t B, int64_t n, int64_t J, const int64_t* m, const double* mat_f,
                            const double* mat_b, const double* c, int device) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1 || n < 1 || n > BATCH_NMAX) return fail(ELLHIP_E_INVALID, "batched LMI: need B >= 1 and 1 <= n <= 128");
    if (J < 1 || J > BATCH_LMI_JMAX) return fail(ELLHIP_E_INVALID, "batched LMI: need 1 <= J <= 8 blocks");
    if (!m || !mat_f) return fail(ELLHIP_E_INVALID, "NULL argument");
    BatchLmiParams L{};
    L.J = (int)J;
    long long sum_mm = 0;
    for (int j = 0; j < (int)J; ++j) {
        if (m[j] < 1 || m[j] > BATCH_LMI_MMAX) return fail(ELLHIP_E_INVALID, "batched LMI: need 1 <= m_j <= 64");
        L.m[j] = (int)m[j];
        L.foff[j] = (int)(sum_mm * n);
        L.boff[j] = (int)sum_mm;
        sum_mm += m[j] * m[j];
        L.mmax = std::max(L.mmax, L.m[j]);
    }
    L.fstride = (int)(sum_mm * n);
    L.bstride = (int)sum_mm;
    L.pm = L.mmax | 1;
    L.has_b = mat_b ? 1 : 0;
    L.has_c = c ? 1 : 0;
    L.nstation = L.J + L.has_c;
    if ((double)B * (double)L.fstride * 8.0 > 100e9) return fail(ELLHIP_E_NOMEM, "batched LMI: the pencils are too large");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched LMI loop has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_batch_lmi* o = new (std::nothrow) ellhip_batch_lmi();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->device = device;
    o->B = B;
    o->n = (int)n;
    o->L = L;
    DeviceGuard guard(device);
    auto bail = [&](int code) {
        ellhip_batch_lmi_destroy(o);
        return code;
    };
    const size_t sB = (size_t)B, sn = (size_t)n;
    // repack: the caller's [block][B][k][a][b] becomes [B][block][a][b][k]
    std::vector<double> pk(sB * (size_t)L.fstride);
    std::vector<double> pb(mat_b ? sB * (size_t)L.bstride : 0);
    size_t src_f = 0, src_b = 0;
    for (int j = 0; j < L.J; ++j) {
        const size_t mm = (size_t)L.m[j] * L.m[j];
        for (size_t b = 0; b < sB; ++b) {
            double* dst = pk.data() + b * (size_t)L.fstride + L.foff[j];
            const double* src = mat_f + src_f + b * sn * mm;
            for (size_t k = 0; k < sn; ++k)
                for (size_t el = 0; el < mm; ++el) dst[el * sn + k] = src[k * mm + el];
            if (mat_b) memcpy(pb.data() + b * (size_t)L.bstride + L.boff[j], mat_b + src_b + b * mm, mm * sizeof(double));
        }
        src_f += sB * sn * mm;
        src_b += sB * mm;
    }
    hipError_t e = hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&o->d_pencil, pk.size() * sizeof(double));
    if (e == hipSuccess && mat_b) e = hipMalloc(&o->d_matb, pb.size() * sizeof(double));
    if (e == hipSuccess && c) e = hipMalloc(&o->d_c, sB * sn * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_idx, sB * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&o->d_gamma, sB * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_xbest, sB * sn * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_niter, sB * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(&o->d_ints, (3 * sB + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&o->d_x, sB * sn * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_grad, sB * sn * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&o->d_beta, sB * sizeof(double));
    if (e != hipSuccess) return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched LMI allocation", e));
    e = hipMemcpy(o->d_pencil, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && mat_b) e = hipMemcpy(o->d_matb, pb.data(), pb.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && c) e = hipMemcpy(o->d_c, c, sB * sn * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = fill_now(o->d_idx, 0xff, sB * sizeof(int), o->stream);  // idx = -1
    if (e == hipSuccess) e = fill_now(o->d_xbest, 0, sB * sn * sizeof(double), o->stream);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched LMI upload", e));
    *out = o;
    return 0;
}

void ellhip_batch_lmi_destroy(ellhip_batch_lmi* o) {
    if (!o) return;
    DeviceGuard guard(o->device);
    if (o->stream) (void)hipStreamSynchronize(o->stream);
    void* bufs[] = {o->d_pencil, o->d_matb, o->d_c, o->d_idx, o->d_gamma, o->d_xbest, o->d_niter, o->d_ints, o->d_x, o->d_grad,
                    o->d_beta};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    if (o->stream) (void)hipStreamDestroy(o->stream);
    delete o;
}

int ellhip_batch_lmi_assess_optim(ellhip_batch_lmi* o, const double* x, double* gamma_inout, double* grad_out, double* beta_out,
                                  int32_t* station_out) {
    if (!o || !x || !gamma_inout || !grad_out || !beta_out || !station_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->device);
    const size_t B = (size_t)o->B, n = (size_t)o->n;
    const int T = o->n <= 64 ? 256 : 128;
    int epw = std::min(64, T / o->n);
    const size_t per_bytes = (batch_lmi_lds_doubles(o->n, o->L.mmax) + n) * sizeof(double);
    while (epw > 1 && (size_t)epw * per_bytes > 64 * 1024) epw -= 1;
    const size_t lds = (size_t)epw * per_bytes;  // at most (2*128 + 64*65 + 64 + 17 + 128) * 8 < 64 KiB for one instance
    const unsigned grid = (unsigned)((o->B + epw - 1) / epw);
    int* d_station = o->d_ints;
    HIPCHK(hipMemcpy(o->d_x, x, B * n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->d_grad, grad_out, B * n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->d_gamma, gamma_inout, B * sizeof(double), hipMemcpyHostToDevice));
#define BATCH_LMI_ASSESS(TT)                                                                                           \
    hipLaunchKernelGGL(k_batch_lmi_assess<TT>, dim3(grid), dim3(TT), lds, o->stream, o->B, o->n, epw, o->L,            \
                       (const double*)o->d_pencil, (const double*)o->d_matb, (const double*)o->d_c,                    \
                       (const double*)o->d_x, o->d_idx, o->d_gamma, o->d_grad, o->d_beta, d_station)
    if (T == 128) BATCH_LMI_ASSESS(128);
    else BATCH_LMI_ASSESS(256);
#undef BATCH_LMI_ASSESS
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(o->stream));
    HIPCHK(hipMemcpy(grad_out, o->d_grad, B * n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(beta_out, o->d_beta, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(gamma_inout, o->d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(station_out, d_station, B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int ellhip_batch_lmi_get_idx(ellhip_batch_lmi* o, int32_t* idx_out) {
    if (!o || !idx_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->device);
    HIPCHK(hipStreamSynchronize(o->stream));
    HIPCHK(hipMemcpy(idx_out, o->d_idx, (size_t)o->B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int ellhip_batch_lmi_set_idx(ellhip_batch_lmi* o, const int32_t* idx) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(o->device);
    HIPCHK(hipStreamSynchronize(o->stream));
    if (!idx) {
        HIPCHK(fill_now(o->d_idx, 0xff, (size_t)o->B * sizeof(int), o->stream));
        return 0;
    }
    for (long long b = 0; b < o->B; ++b)
        if (idx[b] < -1 || idx[b] > o->L.J) return fail(ELLHIP_E_INVALID, "batched LMI: idx must be in -1..J");
    HIPCHK(hipMemcpy(o->d_idx, idx, (size_t)o->B * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

int ellhip_batch_lmi_optim(ellhip_batch* spaces, ellhip_batch_lmi* o, double* gamma_inout, int64_t max_iters, double tol,
                           double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lmi_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out);
}

int ellhip_batch_lmi_feas(ellhip_batch* spaces, ellhip_batch_lmi* o, int64_t max_iters, double tol, double* x_out,
                          int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lmi_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out);
}

int ellhip_batch_lmi_set_chunk(ellhip_batch_lmi* o, int64_t iters) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (iters < 1 || iters > 4096) return fail(ELLHIP_E_INVALID, "batched LMI: chunk must be in 1..4096");
    o->chunk = (int)iters;
    return 0;
}

}  // extern "C"
