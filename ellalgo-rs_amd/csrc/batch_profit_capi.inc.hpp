// batch_profit_capi.inc.hpp -- C ABI of the batched device-resident profit-maximisation loops
// (include/ellhip_batch_profit.h).  Included from ellhip_capi.hip after batch_loop_capi.inc.hpp (the loop state, the launch
// shapes and the one driver, batch_loop_run, through which both LDS engines and both drivers are reached).
//
// Reference: src/oracles/profit_oracle.rs (oracles), src/cutting_plane.rs:286-313, 331-374 (loops).
#include "../../include/ellhip_batch_profit.h"

#include "batch_profit_kernels.hpp"

struct ellhip_batch_profit {
    BatchLoopBuffers loop;     // device, B, n = 2, stream, the loop state
    long long B = 0;
    int kind = 0;
    double* d_cst = nullptr;   // [B][PF_NCONST]
    int* d_idx = nullptr;      // [B] the constraint cursors
    double* d_yd = nullptr;    // [B][2]
    int* d_retry = nullptr;    // [B] the optim_q driver's retry flags; assess_optim_q: the caller's
    double* d_x = nullptr;     // assess: [B][2]
    double* d_vec = nullptr;   // assess: grad [B][2], x_q [B][2]
    double* d_out = nullptr;   // assess: gamma [B], beta [B]
    int* d_flags = nullptr;    // assess: shrunk [B], more_alt [B]
};

namespace {

template <bool Q>
typename BatchProfitOracle<Q>::Args batch_profit_args(const ellhip_batch_profit* o) {
    typename BatchProfitOracle<Q>::Args A;
    A.cst = o->d_cst;
    A.idx = o->d_idx;
    A.yd = o->d_yd;
    A.retry = o->d_retry;
    A.kind = o->kind;
    return A;
}

constexpr BatchLoopWords BATCH_PROFIT_WORDS{"profit", "n", " (a profit problem has n = 2)"};

// q: the entry point is an optim_q one, which takes the discrete kind and no other
int batch_profit_run(ellhip_batch* s, ellhip_batch_profit* o, bool q, double* gamma_inout, int64_t max_iters, double tol,
                     double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out,
                     BatchLoopEngine engine) {
    if (!s || !o || !gamma_inout || !has_best_out || !niter_out || !status_out)
        return fail(ELLHIP_E_INVALID, "NULL argument");
    if (q != (o->kind == PROFIT_DISCRETE))
        return fail(ELLHIP_E_INVALID, q ? "batched profit loop: the optim_q entry points take the discrete kind only"
                                        : "batched profit loop: the discrete kind runs under the optim_q entry points only");
    if (q)
        return batch_loop_run<BatchProfitOracle<true>, BATCH_DRIVER_OPTIM_Q, false>(
            s, o->loop, batch_profit_args<true>(o), BATCH_PROFIT_WORDS, engine, 0, gamma_inout, max_iters, tol, x_best_out,
            has_best_out, niter_out, status_out, o->d_retry);
    return batch_loop_run<BatchProfitOracle<false>, BATCH_DRIVER_OPTIM, false>(
        s, o->loop, batch_profit_args<false>(o), BATCH_PROFIT_WORDS, engine, 0, gamma_inout, max_iters, tol, x_best_out,
        has_best_out, niter_out, status_out);
}

int batch_profit_assess(ellhip_batch_profit* o, bool q, const double* x, double* gamma_inout, const int32_t* retry,
                        double* grad_out, double* beta_out, int32_t* shrunk_out, double* x_q_out, int32_t* more_alt_out) {
    if (!o || !x || !gamma_inout || !grad_out || (q && !retry)) return fail(ELLHIP_E_INVALID, "NULL argument");
    if (q != (o->kind == PROFIT_DISCRETE))
        return fail(ELLHIP_E_INVALID, q ? "batched profit: assess_optim_q takes the discrete kind only"
                                        : "batched profit: the discrete kind has assess_optim_q only");
    DeviceGuard guard(o->loop.device);
    const size_t B = (size_t)o->B;
    const int T = 256;
    const size_t lds = (size_t)(T / 2) * (batch_profit_lds_doubles() + 2) * sizeof(double);  // 27 KiB
    const unsigned grid = (unsigned)((o->B + T / 2 - 1) / (T / 2));
    double* d_gamma = o->d_out;
    double* d_beta = o->d_out + B;
    double* d_grad = o->d_vec;
    double* d_xq = o->d_vec + 2 * B;
    int* d_shrunk = o->d_flags;
    int* d_more = o->d_flags + B;
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(o->d_x, x, 2 * B * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_gamma, gamma_inout, B * sizeof(double), hipMemcpyHostToDevice));
    if (q) {
        static_assert(sizeof(int) == sizeof(int32_t), "retry is copied as it is");
        HIPCHK(hipMemcpy(o->d_retry, retry, B * sizeof(int), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_batch_profit_assess<true>, dim3(grid), dim3(T), lds, o->loop.stream, o->B,
                           batch_profit_args<true>(o), (const double*)o->d_x, d_gamma, (const int*)o->d_retry, d_grad, d_beta,
                           d_shrunk, d_xq, d_more);
    } else {
        hipLaunchKernelGGL(k_batch_profit_assess<false>, dim3(grid), dim3(T), lds, o->loop.stream, o->B,
                           batch_profit_args<false>(o), (const double*)o->d_x, d_gamma, (const int*)nullptr, d_grad, d_beta,
                           d_shrunk, d_xq, d_more);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(gamma_inout, d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(grad_out, d_grad, 2 * B * sizeof(double), hipMemcpyDeviceToHost));
    if (beta_out) HIPCHK(hipMemcpy(beta_out, d_beta, B * sizeof(double), hipMemcpyDeviceToHost));
    if (shrunk_out) HIPCHK(hipMemcpy(shrunk_out, d_shrunk, B * sizeof(int), hipMemcpyDeviceToHost));
    if (q && x_q_out) HIPCHK(hipMemcpy(x_q_out, d_xq, 2 * B * sizeof(double), hipMemcpyDeviceToHost));
    if (q && more_alt_out) HIPCHK(hipMemcpy(more_alt_out, d_more, B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

int ellhip_batch_profit_create(ellhip_batch_profit** out, int64_t B, int32_t kind, const double* params,
                               const double* elasticities, const double* price_out, const double* vparams, int device) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1 || B > (1 << 24)) return fail(ELLHIP_E_INVALID, "batched profit: need 1 <= B <= 2^24");
    if (kind != PROFIT_PLAIN && kind != PROFIT_ROBUST && kind != PROFIT_DISCRETE)
        return fail(ELLHIP_E_INVALID, "batched profit: kind must be ELLHIP_PROFIT_PLAIN, _ROBUST or _DISCRETE");
    if (!params || !elasticities || !price_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    if ((kind == PROFIT_ROBUST) != (vparams != nullptr))
        return fail(ELLHIP_E_INVALID, "batched profit: vparams goes with the robust kind and with no other");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched profit loop has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_batch_profit* o = new (std::nothrow) ellhip_batch_profit();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->B = B;
    o->kind = kind;
    DeviceGuard guard(device);
    auto bail = [&](int code) {
        ellhip_batch_profit_destroy(o);
        return code;
    };
    const size_t sB = (size_t)B;
    // ProfitOracle::new (:19-33), ProfitRbOracle::new (:89-108): the logarithms through ell_log, as the kernels' are
    std::vector<double> cst(sB * PF_NCONST);
    for (size_t b = 0; b < sB; ++b) {
        double* c = cst.data() + b * PF_NCONST;
        double unit_price = params[3 * b], limit = params[3 * b + 2], shift = 0.0;
        const double scale = params[3 * b + 1];
        c[PFC_UIE] = c[PFC_UIE + 1] = 0.0;
        if (kind == PROFIT_ROBUST) {
            const double* e = vparams + 5 * b;
            c[PFC_UIE] = e[0];
            c[PFC_UIE + 1] = e[1];
            unit_price = unit_price - e[2];
            limit = limit - e[3];
            shift = e[4];
        }
        c[PFC_LOG_P_SCALE] = ell_log(unit_price * scale);
        c[PFC_LOG_K] = ell_log(limit);
        c[PFC_PRICE] = kind == PROFIT_ROBUST ? price_out[2 * b] + shift : price_out[2 * b];
        c[PFC_PRICE + 1] = kind == PROFIT_ROBUST ? price_out[2 * b + 1] + shift : price_out[2 * b + 1];
        c[PFC_A] = elasticities[2 * b];
        c[PFC_A + 1] = elasticities[2 * b + 1];
    }
    hipError_t e = batch_loop_alloc(o->loop, device, B, 2);
    if (e == hipSuccess) e = o->loop.mem.device(o->d_cst, sB * PF_NCONST * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_idx, sB * sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_yd, 2 * sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_retry, sB * sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_x, 2 * sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_vec, 4 * sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_out, 2 * sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_flags, 2 * sB * sizeof(int));
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched profit allocation", e));
    e = fill_now(o->d_idx, 0xff, sB * sizeof(int), o->loop.stream);  // idx = -1                                  :24
    if (e == hipSuccess) e = fill_now(o->d_yd, 0, 2 * sB * sizeof(double), o->loop.stream);  //                   :136
    if (e == hipSuccess) e = fill_now(o->d_retry, 0, sB * sizeof(int), o->loop.stream);
    if (e == hipSuccess) e = hipMemcpy(o->d_cst, cst.data(), sB * PF_NCONST * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched profit upload", e));
    *out = o;
    return 0;
}

void ellhip_batch_profit_destroy(ellhip_batch_profit* o) {
    if (!o) return;
    DeviceGuard guard(o->loop.device);
    batch_loop_free(o->loop);
    delete o;
}

int ellhip_batch_profit_set_chunk(ellhip_batch_profit* o, int64_t iters) {
    return batch_loop_set_chunk(o ? &o->loop : nullptr, iters, "batched profit");
}

int ellhip_batch_profit_assess_optim(ellhip_batch_profit* o, const double* x, double* gamma_inout, double* grad_out,
                                     double* beta_out, int32_t* shrunk_out) {
    return batch_profit_assess(o, false, x, gamma_inout, nullptr, grad_out, beta_out, shrunk_out, nullptr, nullptr);
}

int ellhip_batch_profit_assess_optim_q(ellhip_batch_profit* o, const double* x, double* gamma_inout, const int32_t* retry,
                                       double* grad_out, double* beta_out, int32_t* shrunk_out, double* x_q_out,
                                       int32_t* more_alt_out) {
    return batch_profit_assess(o, true, x, gamma_inout, retry, grad_out, beta_out, shrunk_out, x_q_out, more_alt_out);
}

int ellhip_batch_profit_optim(ellhip_batch* s, ellhip_batch_profit* o, double* gamma_inout, int64_t max_iters, double tol,
                              double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out) {
    return batch_profit_run(s, o, false, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                            BATCH_ENGINE_LDS);
}

int ellhip_batch_profit_optim_stable(ellhip_batch* s, ellhip_batch_profit* o, double* gamma_inout, int64_t max_iters,
                                     double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                     int32_t* status_out) {
    return batch_profit_run(s, o, false, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                            BATCH_ENGINE_LDS_STABLE);
}

int ellhip_batch_profit_optim_q(ellhip_batch* s, ellhip_batch_profit* o, double* gamma_inout, int64_t max_iters, double tol,
                                double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out) {
    return batch_profit_run(s, o, true, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                            BATCH_ENGINE_LDS);
}

int ellhip_batch_profit_optim_q_stable(ellhip_batch* s, ellhip_batch_profit* o, double* gamma_inout, int64_t max_iters,
                                       double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                       int32_t* status_out) {
    return batch_profit_run(s, o, true, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                            BATCH_ENGINE_LDS_STABLE);
}

int ellhip_math_eval(int32_t fn, int64_t count, const double* x, double* out, int device) {
    if (!x || !out || count < 0 || (fn != 0 && fn != 1)) return fail(ELLHIP_E_INVALID, "bad argument");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    if (count == 0) return 0;
    DeviceGuard guard(device);
    Allocs tmp;  // (freed on every return path)
    double* d_x = nullptr;
    double* d_out = nullptr;
    const size_t bytes = (size_t)count * sizeof(double);
    HIPCHK(tmp.device(d_x, bytes));
    HIPCHK(tmp.device(d_out, bytes));
    HIPCHK(hipMemcpy(d_x, x, bytes, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)std::min<long long>((count + 255) / 256, 4096);
    hipLaunchKernelGGL(k_math_eval, dim3(grid), dim3(256), 0, 0, (int)fn, (long long)count, (const double*)d_x, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
