// batch_maxcut_capi.inc.hpp -- C ABI of the batched device-resident max-cut cutting-plane loops
// (include/ellhip_batch_maxcut.h).  Included from ellhip_capi.hip after batch_loop_capi.inc.hpp (the loop state, the launch
// shapes and the one driver, batch_loop_run, through which all four engines are reached).
//
// Reference: src/oracles/maxcut_oracle.rs:4-50 (oracle), src/cutting_plane.rs:286-313 (loop).
#include "../../include/ellhip_batch_maxcut.h"

#include "batch_maxcut_kernels.hpp"

struct ellhip_batch_maxcut {
    BatchLoopBuffers loop;    // device, B, n, stream, the loop state
    long long B = 0;
    int n = 0;
    int shared = 0;
    double* d_W = nullptr;    // [ntab][n][n] row-major, ntab = 1 (shared) or B
    double* d_WT = nullptr;   // the transposes; == d_W when every table is symmetric to the bit
    double* d_x = nullptr;    // assess: [B][n]
    double* d_grad = nullptr; // assess: [B][n]
    double* d_out = nullptr;  // assess: gamma [B], beta [B], shrunk [B], cut_value [B]
};

namespace {

BatchMaxcutOracle::Args batch_maxcut_args(const ellhip_batch_maxcut* o) {
    BatchMaxcutOracle::Args A;
    A.W = o->d_W;
    A.WT = o->d_WT;
    A.tab_stride = o->shared ? 0 : (long long)o->n * o->n;
    return A;
}

// w[i][j] and w[j][i] have the same bits in every table
bool batch_maxcut_symmetric(const double* w, size_t ntab, size_t n) {
    for (size_t t = 0; t < ntab; ++t) {
        const double* a = w + t * n * n;
        for (size_t i = 0; i < n; ++i)
            for (size_t j = i + 1; j < n; ++j)
                if (memcmp(a + i * n + j, a + j * n + i, sizeof(double)) != 0) return false;
    }
    return true;
}

int batch_maxcut_run(ellhip_batch* s, ellhip_batch_maxcut* o, double* gamma_inout, int64_t max_iters, double tol,
                     double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out,
                     BatchLoopEngine engine) {
    if (!s || !o || !gamma_inout || !has_best_out || !niter_out || !status_out)
        return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_loop_run<BatchMaxcutOracle>(s, o->loop, batch_maxcut_args(o), BatchLoopWords{"max-cut", "n", ""}, engine, 0,
                                             gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out);
}

}  // namespace

extern "C" {

int ellhip_batch_maxcut_create(ellhip_batch_maxcut** out, int64_t B, int64_t n, const double* weights,
                               int32_t shared_weights, int device) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1 || B > (1 << 24)) return fail(ELLHIP_E_INVALID, "batched max-cut: need 1 <= B <= 2^24");
    if (n < 1 || n > BATCH_STREAMED_NMAX)
        return fail(ELLHIP_E_INVALID, ("batched max-cut: need 1 <= n <= " + std::to_string(BATCH_STREAMED_NMAX)).c_str());
    if (!weights) return fail(ELLHIP_E_INVALID, "NULL argument");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched max-cut loop has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_batch_maxcut* o = new (std::nothrow) ellhip_batch_maxcut();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->B = B;
    o->n = (int)n;
    o->shared = shared_weights != 0;
    DeviceGuard guard(device);
    auto bail = [&](int code) {
        ellhip_batch_maxcut_destroy(o);
        return code;
    };
    const size_t sB = (size_t)B, sn = (size_t)n;
    const size_t ntab = o->shared ? 1 : sB;
    const size_t tbytes = ntab * sn * sn * sizeof(double);
    const bool one = batch_maxcut_symmetric(weights, ntab, sn);
    hipError_t e = batch_loop_alloc(o->loop, device, B, o->n);
    if (e == hipSuccess) e = o->loop.mem.device(o->d_W, tbytes);
    if (e == hipSuccess && !one) e = o->loop.mem.device(o->d_WT, tbytes);
    if (e == hipSuccess) e = o->loop.mem.device(o->d_x, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_grad, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_out, 4 * sB * sizeof(double));
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched max-cut allocation", e));
    // the tables, taken as one [ntab * n][n] matrix: bounded slabs of its rows go up into the row-major copy, and each slab
    // is transposed on the device from there (no staging buffer, no host transpose)
    if (one) o->d_WT = o->d_W;
    const long long total = (long long)ntab * n;
    const long long slab_tabs = std::max<long long>(1, (64LL << 20) / (n * n * 8));  // whole tables: a tile never straddles two
    const long long slab_rows = slab_tabs * n;
    for (long long r0 = 0; r0 < total && e == hipSuccess; r0 += slab_rows) {
        const long long rows = std::min(total - r0, slab_rows);
        e = hipMemcpyAsync(o->d_W + (size_t)r0 * sn, weights + (size_t)r0 * sn, (size_t)rows * sn * sizeof(double),
                           hipMemcpyHostToDevice, o->loop.stream);
        if (e != hipSuccess || one) continue;
        const long long tiles = ((n + BATCH_MAXCUT_TILE - 1) / BATCH_MAXCUT_TILE) * ((rows + BATCH_MAXCUT_TILE - 1) / BATCH_MAXCUT_TILE);
        hipLaunchKernelGGL(k_batch_maxcut_transpose, dim3((unsigned)std::min<long long>(tiles, 4096)), dim3(256), 0,
                           o->loop.stream, (const double*)(o->d_W + (size_t)r0 * sn), rows, (long long)n,
                           o->d_WT + (size_t)r0 * sn);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(o->loop.stream);  // the caller's buffer is free again
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched max-cut table upload", e));
    *out = o;
    return 0;
}

void ellhip_batch_maxcut_destroy(ellhip_batch_maxcut* o) {
    if (!o) return;
    DeviceGuard guard(o->loop.device);
    batch_loop_free(o->loop);
    delete o;
}

int ellhip_batch_maxcut_set_chunk(ellhip_batch_maxcut* o, int64_t iters) {
    return batch_loop_set_chunk(o ? &o->loop : nullptr, iters, "batched max-cut");
}

int ellhip_batch_maxcut_assess_optim(ellhip_batch_maxcut* o, const double* x, double* gamma_inout, double* grad_out,
                                     double* beta_out, int32_t* shrunk_out, double* cut_value_out) {
    if (!o || !x || !gamma_inout || !grad_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->loop.device);
    const size_t B = (size_t)o->B, n = (size_t)o->n;
    const size_t per = batch_maxcut_lds_doubles(o->n) + n;
    // past the LDS engine's n (batch_row_shape has no instance per workgroup to offer): one instance per workgroup, n threads
    // rounded up to whole waves, as the streamed engine shapes its own
    const bool wide = o->n > BATCH_NMAX;
    const BatchRowShape sh = batch_row_shape(o->n, per);
    const int T = wide ? (o->n + 63) / 64 * 64 : sh.T, epw = wide ? 1 : sh.epw;
    const size_t lds = (size_t)epw * per * sizeof(double);  // under 9 KiB packed, 32.1 KiB at n = 1024
    const unsigned grid = (unsigned)((o->B + epw - 1) / epw);
    const BatchMaxcutOracle::Args A = batch_maxcut_args(o);
    double* d_gamma = o->d_out;
    double* d_beta = o->d_out + B;
    double* d_shrunk = o->d_out + 2 * B;
    double* d_cut = o->d_out + 3 * B;
    HIPCHK(hipMemcpy(o->d_x, x, B * n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_gamma, gamma_inout, B * sizeof(double), hipMemcpyHostToDevice));
#define BATCH_MAXCUT_ASSESS(TT)                                                                                        \
    hipLaunchKernelGGL(k_batch_maxcut_assess<TT>, dim3(grid), dim3(T), lds, o->loop.stream, o->B, o->n, epw, A,        \
                       (const double*)o->d_x, d_gamma, o->d_grad, d_beta, d_shrunk, d_cut)
    if (wide) BATCH_MAXCUT_ASSESS(1024);  // (the template argument bounds the block; the block is T threads)
    else if (T == 128) BATCH_MAXCUT_ASSESS(128);
    else BATCH_MAXCUT_ASSESS(256);
#undef BATCH_MAXCUT_ASSESS
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(gamma_inout, d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(grad_out, o->d_grad, B * n * sizeof(double), hipMemcpyDeviceToHost));
    if (beta_out) HIPCHK(hipMemcpy(beta_out, d_beta, B * sizeof(double), hipMemcpyDeviceToHost));
    if (cut_value_out) HIPCHK(hipMemcpy(cut_value_out, d_cut, B * sizeof(double), hipMemcpyDeviceToHost));
    if (shrunk_out) {
        std::vector<double> sh_d(B);
        HIPCHK(hipMemcpy(sh_d.data(), d_shrunk, B * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) shrunk_out[b] = sh_d[b] != 0.0;
    }
    return 0;
}

int ellhip_batch_maxcut_optim(ellhip_batch* s, ellhip_batch_maxcut* o, double* gamma_inout, int64_t max_iters, double tol,
                              double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out) {
    return batch_maxcut_run(s, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out, BATCH_ENGINE_LDS);
}

int ellhip_batch_maxcut_optim_stable(ellhip_batch* s, ellhip_batch_maxcut* o, double* gamma_inout, int64_t max_iters,
                                     double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                     int32_t* status_out) {
    return batch_maxcut_run(s, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                            BATCH_ENGINE_LDS_STABLE);
}

int ellhip_batch_maxcut_optim_streamed(ellhip_batch* s, ellhip_batch_maxcut* o, double* gamma_inout, int64_t max_iters,
                                       double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                       int32_t* status_out) {
    return batch_maxcut_run(s, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                            BATCH_ENGINE_STREAMED);
}

int ellhip_batch_maxcut_optim_streamed_stable(ellhip_batch* s, ellhip_batch_maxcut* o, double* gamma_inout,
                                              int64_t max_iters, double tol, double* x_best_out, int32_t* has_best_out,
                                              int64_t* niter_out, int32_t* status_out) {
    return batch_maxcut_run(s, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                            BATCH_ENGINE_STREAMED_STABLE);
}

}  // extern "C"
