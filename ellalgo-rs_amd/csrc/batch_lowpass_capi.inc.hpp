// batch_lowpass_capi.inc.hpp -- C ABI of the batched device-resident low-pass filter design loop
// (include/ellhip_batch_lowpass.h).  Included at the end of ellhip_capi.hip, after lowpass_capi.inc.hpp (it builds the
// table with the same lp_fill_rows) and batch_loop_capi.inc.hpp (the loop state, the launch shapes and the driver).
//
// Reference: src/oracles/lowpass_oracle.rs:22-151 (oracle), src/cutting_plane.rs:205-227, 286-313 (loops).
#include "../../include/ellhip_batch_lowpass.h"

#include "batch_lowpass_kernels.hpp"

struct ellhip_batch_lowpass {
    BatchLoopBuffers loop;        // device, B, n, stream, the loop state (d_gamma: also assess_optim)
    long long B = 0;
    int n = 0;
    int mdim = 0;
    std::vector<int> bands;       // host copy of [B][2]: nwpass, nwstop (reset, state)
    double* d_spec = nullptr;     // [15 n][n]
    double* d_specT = nullptr;    // [n][15 n]
    int* d_bands = nullptr;       // [B][2]
    double* d_lims = nullptr;     // [B][2]: lp_sq, up_sq
    int* d_cursor = nullptr;      // [B][4]: idx1, idx2, idx3, more_alt
    int* d_kmax = nullptr;        // [B]
    double* d_fmax = nullptr;     // [B]
    double* d_spsq = nullptr;     // [B]
    double* d_x = nullptr;        // assess: [B][n]
    double* d_grad = nullptr;     // assess: [B][n]
    double* d_beta = nullptr;     // assess: beta0 [B], beta1 [B]
    int* d_aints = nullptr;       // assess: has_beta1 [B], answer [B]
};

namespace {

BatchLpOracle::Args batch_lowpass_args(const ellhip_batch_lowpass* o) {
    BatchLpOracle::Args A;
    A.spec = o->d_spec;
    A.specT = o->d_specT;
    A.bands = o->d_bands;
    A.lims = o->d_lims;
    A.cursor = o->d_cursor;
    A.kmax = o->d_kmax;
    A.fmax = o->d_fmax;
    A.spsq = o->d_spsq;
    A.mdim = o->mdim;
    return A;
}

// cursors, fmax and kmax as LowpassOracle::new leaves them (src/oracles/lowpass_oracle.rs:41-52)
int batch_lowpass_fresh(ellhip_batch_lowpass* o) {
    const size_t B = (size_t)o->B;
    std::vector<int> cur(4 * B), kmax(B, -1);
    std::vector<double> fmax(B, -__builtin_inf());
    for (size_t b = 0; b < B; ++b) {
        cur[4 * b] = -1;
        cur[4 * b + 1] = o->bands[2 * b] - 1;
        cur[4 * b + 2] = o->bands[2 * b + 1] - 1;
        cur[4 * b + 3] = 1;
    }
    HIPCHK(hipMemcpy(o->d_cursor, cur.data(), 4 * B * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->d_kmax, kmax.data(), B * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->d_fmax, fmax.data(), B * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

// the loops of all four headers (ellhip_batch_lowpass.h, ellhip_batch_stable_loops.h, ellhip_batch_lowpass_streamed.h,
// ellhip_batch_lowpass_streamed_stable.h) on `engine`
int batch_lowpass_run(ellhip_batch* s, ellhip_batch_lowpass* o, int feas, double* gamma_inout, int64_t max_iters,
                      double tol, double* x_out, int32_t* has_out, int64_t* niter_out, int32_t* status_out,
                      BatchLoopEngine engine) {
    if (!s || !o || !has_out || !niter_out || !status_out || (!feas && !gamma_inout))
        return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_loop_run<BatchLpOracle>(s, o->loop, batch_lowpass_args(o), {"lowpass", "n", ""}, engine, feas, gamma_inout,
                                         max_iters, tol, x_out, has_out, niter_out, status_out);
}

// one oracle call per problem; ans[B] = BLP_*
int batch_lowpass_assess(ellhip_batch_lowpass* o, int optim, const double* x, double* gamma_inout, double* grad_out,
                         double* beta0, int32_t* has_beta1, double* beta1, std::vector<int>& ans) {
    if (!o || !x || !grad_out || !beta0 || !has_beta1 || !beta1 || (optim && !gamma_inout))
        return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->loop.device);
    const size_t B = (size_t)o->B, n = (size_t)o->n;
    const size_t per = batch_lowpass_lds_doubles(o->n) + n;
    // past the LDS engine's n (batch_row_shape has no instance per workgroup to offer): one instance per workgroup, n threads
    // rounded up to whole waves, as the streamed engine shapes its own
    const bool wide = o->n > BATCH_NMAX;
    const BatchRowShape sh = batch_row_shape(o->n, per);
    const int T = wide ? (o->n + 63) / 64 * 64 : sh.T, epw = wide ? 1 : sh.epw;
    const size_t lds = (size_t)epw * per * sizeof(double);  // at most 64 * 29 * 8 bytes, or 16.2 KiB at n = 1024
    const unsigned grid = (unsigned)((o->B + epw - 1) / epw);
    double* d_beta0 = o->d_beta;
    double* d_beta1 = o->d_beta + B;
    int* d_hb1 = o->d_aints;
    int* d_ans = o->d_aints + B;
    const BatchLpOracle::Args A = batch_lowpass_args(o);
    HIPCHK(hipMemcpy(o->d_x, x, B * n * sizeof(double), hipMemcpyHostToDevice));
    if (optim) HIPCHK(hipMemcpy(o->loop.d_gamma, gamma_inout, B * sizeof(double), hipMemcpyHostToDevice));
#define BATCH_LP_ASSESS(TT)                                                                                            \
    hipLaunchKernelGGL(k_batch_lowpass_assess<TT>, dim3(grid), dim3(T), lds, o->loop.stream, o->B, o->n, epw, optim,   \
                       A, o->loop.d_gamma, (const double*)o->d_x, o->d_grad, d_beta0, d_hb1, d_beta1, d_ans)
    if (wide) BATCH_LP_ASSESS(1024);  // (the template argument bounds the block; the block is T threads)
    else if (T == 128) BATCH_LP_ASSESS(128);
    else BATCH_LP_ASSESS(256);
#undef BATCH_LP_ASSESS
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    std::vector<double> g(B * n), b0(B), b1(B);
    std::vector<int> hb1(B);
    ans.resize(B);
    HIPCHK(hipMemcpy(ans.data(), d_ans, B * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g.data(), o->d_grad, B * n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(b0.data(), d_beta0, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(b1.data(), d_beta1, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hb1.data(), d_hb1, B * sizeof(int), hipMemcpyDeviceToHost));
    if (optim) HIPCHK(hipMemcpy(gamma_inout, o->loop.d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {  // a problem without a cut leaves its outputs as the caller had them
        if (ans[b] != BLP_CUT && ans[b] != BLP_SHRUNK) continue;
        memcpy(grad_out + b * n, g.data() + b * n, n * sizeof(double));
        beta0[b] = b0[b];
        has_beta1[b] = hb1[b];
        beta1[b] = b1[b];
    }
    return 0;
}

// nmax: 128 for the LDS engine's constructor, 1024 for the streamed one (batch_lowpass_streamed_capi.inc.hpp)
int batch_lowpass_create(ellhip_batch_lowpass** out, int64_t B, int64_t n, const double* wpass, const double* wstop,
                         const double* lp_sq, const double* up_sq, const double* sp_sq, const double* spectrum, int device,
                         int nmax) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1 || n < 1 || n > nmax)
        return fail(ELLHIP_E_INVALID, ("batched lowpass: need B >= 1 and 1 <= n <= " + std::to_string(nmax)).c_str());
    if (B > (1 << 24)) return fail(ELLHIP_E_INVALID, "batched lowpass: B too large");
    if (!wpass || !wstop || !lp_sq || !up_sq || !sp_sq) return fail(ELLHIP_E_INVALID, "NULL argument");
    const long long mdim = 15 * n;  //                                      src/oracles/lowpass_oracle.rs:24
    const size_t sB = (size_t)B, sn = (size_t)n;
    std::vector<int> bands(2 * sB);
    std::vector<double> lims(2 * sB);
    for (size_t b = 0; b < sB; ++b) {
        if (wpass[b] > wstop[b]) return fail(ELLHIP_E_INVALID, "batched lowpass: wpass > wstop");
        const double fpass = std::floor(wpass[b] * (double)(mdim - 1));  //   :36
        const double fstop = std::floor(wstop[b] * (double)(mdim - 1));  //   :37
        if (!(fpass >= 0.0 && fpass <= fstop && fstop <= (double)(mdim - 1)))  // (NaN fails too)
            return fail(ELLHIP_E_INVALID, "batched lowpass: band edges must satisfy 0 <= wpass <= wstop <= 1");
        const long long nwpass = (long long)fpass + 1, nwstop = (long long)fstop + 1;
        bands[2 * b] = (int)nwpass;
        bands[2 * b + 1] = (int)nwstop;
        lims[2 * b] = lp_sq[b];
        lims[2 * b + 1] = up_sq[b];
    }
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched lowpass loop has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_batch_lowpass* o = new (std::nothrow) ellhip_batch_lowpass();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->B = B;
    o->n = (int)n;
    o->mdim = (int)mdim;
    o->bands = bands;
    DeviceGuard guard(device);
    auto bail = [&](int code) {
        ellhip_batch_lowpass_destroy(o);
        return code;
    };
    // the table: the caller's own or computed with the host libm exactly as LowpassOracle::new does (:25-34), and its
    // transpose
    const size_t tab = (size_t)mdim * sn;
    std::vector<double> rows(tab), cols(tab);
    if (spectrum) memcpy(rows.data(), spectrum, tab * sizeof(double));
    else lp_fill_rows(rows.data(), (long long)n, mdim, 0, mdim);
    for (size_t r = 0; r < (size_t)mdim; ++r)
        for (size_t j = 0; j < sn; ++j) cols[j * (size_t)mdim + r] = rows[r * sn + j];
    hipError_t e = batch_loop_alloc(o->loop, device, B, (int)n);
    if (e == hipSuccess) e = o->loop.mem.device(o->d_spec, tab * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_specT, tab * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_bands, 2 * sB * sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_lims, 2 * sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_cursor, 4 * sB * sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_kmax, sB * sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_fmax, sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_spsq, sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_x, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_grad, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_beta, 2 * sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_aints, 2 * sB * sizeof(int));
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched lowpass allocation", e));
    e = hipMemcpy(o->d_spec, rows.data(), tab * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_specT, cols.data(), tab * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_bands, bands.data(), 2 * sB * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_lims, lims.data(), 2 * sB * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_spsq, sp_sq, sB * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->loop.d_gamma, sp_sq, sB * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = fill_now(o->d_grad, 0, sB * sn * sizeof(double), o->loop.stream);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched lowpass upload", e));
    const int rc = batch_lowpass_fresh(o);
    if (rc) return bail(rc);
    *out = o;
    return 0;
}

}  // namespace

extern "C" {

int ellhip_batch_lowpass_create(ellhip_batch_lowpass** out, int64_t B, int64_t n, const double* wpass, const double* wstop,
                                const double* lp_sq, const double* up_sq, const double* sp_sq, const double* spectrum,
                                int device) {
    return batch_lowpass_create(out, B, n, wpass, wstop, lp_sq, up_sq, sp_sq, spectrum, device, BATCH_NMAX);
}

void ellhip_batch_lowpass_destroy(ellhip_batch_lowpass* o) {
    if (!o) return;
    DeviceGuard guard(o->loop.device);
    batch_loop_free(o->loop);
    delete o;
}

int ellhip_batch_lowpass_assess_feas(ellhip_batch_lowpass* o, const double* x, double* grad_out, double* beta0,
                                     int32_t* has_beta1, double* beta1, int32_t* cut_out) {
    if (!cut_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    std::vector<int> ans;
    const int rc = batch_lowpass_assess(o, 0, x, nullptr, grad_out, beta0, has_beta1, beta1, ans);
    if (rc) return rc;
    for (size_t b = 0; b < ans.size(); ++b) cut_out[b] = ans[b] == BLP_CUT ? 1 : 0;
    return 0;
}

int ellhip_batch_lowpass_assess_optim(ellhip_batch_lowpass* o, const double* x, double* gamma_inout, double* grad_out,
                                      double* beta0, int32_t* has_beta1, double* beta1, int32_t* shrunk_out,
                                      int32_t* rc_out) {
    if (!shrunk_out || !rc_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    std::vector<int> ans;
    const int rc = batch_lowpass_assess(o, 1, x, gamma_inout, grad_out, beta0, has_beta1, beta1, ans);
    if (rc) return rc;
    for (size_t b = 0; b < ans.size(); ++b) {
        shrunk_out[b] = ans[b] == BLP_SHRUNK ? 1 : 0;
        rc_out[b] = (ans[b] == BLP_CUT || ans[b] == BLP_SHRUNK) ? 1 : ELLHIP_E_STATE;
    }
    return 0;
}

int ellhip_batch_lowpass_state(ellhip_batch_lowpass* o, int32_t* ints7, double* doubles2) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(o->loop.device);
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    const size_t B = (size_t)o->B;
    if (ints7) {
        std::vector<int> cur(4 * B), kmax(B);
        HIPCHK(hipMemcpy(cur.data(), o->d_cursor, 4 * B * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(kmax.data(), o->d_kmax, B * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) {
            int32_t* r = ints7 + 7 * b;
            r[0] = cur[4 * b + 3];
            r[1] = cur[4 * b];
            r[2] = cur[4 * b + 1];
            r[3] = cur[4 * b + 2];
            r[4] = kmax[b];
            r[5] = o->bands[2 * b];
            r[6] = o->bands[2 * b + 1];
        }
    }
    if (doubles2) {
        std::vector<double> fmax(B), spsq(B);
        HIPCHK(hipMemcpy(fmax.data(), o->d_fmax, B * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(spsq.data(), o->d_spsq, B * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) {
            doubles2[2 * b] = fmax[b];
            doubles2[2 * b + 1] = spsq[b];
        }
    }
    return 0;
}

int ellhip_batch_lowpass_reset(ellhip_batch_lowpass* o) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(o->loop.device);
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    return batch_lowpass_fresh(o);
}

int ellhip_batch_lowpass_get_spectrum(ellhip_batch_lowpass* o, double* out) {
    if (!o || !out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->loop.device);
    HIPCHK(hipMemcpy(out, o->d_spec, (size_t)o->mdim * (size_t)o->n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int ellhip_batch_lowpass_optim(ellhip_batch* spaces, ellhip_batch_lowpass* o, double* gamma_inout, int64_t max_iters,
                               double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                               int32_t* status_out) {
    return batch_lowpass_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                             BATCH_ENGINE_LDS);
}

int ellhip_batch_lowpass_feas(ellhip_batch* spaces, ellhip_batch_lowpass* o, int64_t max_iters, double tol, double* x_out,
                              int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lowpass_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                             BATCH_ENGINE_LDS);
}

int ellhip_batch_lowpass_set_chunk(ellhip_batch_lowpass* o, int64_t iters) {
    return batch_loop_set_chunk(o ? &o->loop : nullptr, iters, "batched lowpass");
}

}  // extern "C"
