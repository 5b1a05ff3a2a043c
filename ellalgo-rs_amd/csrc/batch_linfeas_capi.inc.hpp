// batch_linfeas_capi.inc.hpp -- C ABI of the batched linear feasibility oracles with a movable target and of the
// device-resident bsearch over them (include/ellhip_batch_bsearch.h).  Included from ellhip_capi.hip after
// batch_loop_capi.inc.hpp: the _feas entry points go through its driver, batch_loop_run; the bsearch entry points launch
// k_batch_bsearch, which has a host loop of its own because its stop state is the bisection's, not the loop's.  That host
// loop (batch_bsearch_drive), the argument checks and the constructor are shared with the streamed entry points of
// batch_linfeas_streamed_capi.inc.hpp.
//
// Reference: src/example3.rs (oracle), src/cutting_plane.rs:205-227 (cutting_plane_feas), :403-419 (BSearchAdaptor),
// :441-466 (bsearch).
#include "../../include/ellhip_batch_bsearch.h"

#include "batch_linfeas_kernels.hpp"
#include "batch_linfeas_streamed_kernels.hpp"

struct ellhip_batch_linfeas {
    BatchLoopBuffers loop;       // device, B, n, stream, the loop state of the _feas entry points
    long long B = 0;
    int n = 0, J = 0;
    int shared = 0;
    double* d_a = nullptr;       // [J][n] or [B][J][n]
    double* d_c = nullptr;       // [J] or [B][J]
    int* d_idx = nullptr;        // [B] the cursors
    double* d_target = nullptr;  // [B]
    double* d_x = nullptr;       // assess: [B][n]
    double* d_grad = nullptr;    // assess: [B][n]
    double* d_beta = nullptr;    // assess: [B]
    int* d_cut = nullptr;        // assess: [B]
    // bsearch, allocated by the first call
    double* d_bs = nullptr;      // [B][BSS_N] the bisection state (the LDS engines use [B][BS_N] of it)
    int* d_bs_nstopped = nullptr;
    double* d_pQ = nullptr;      // the probe's space: [B][n][n], [B][n], [B], [B]
    double* d_pxc = nullptr;
    double* d_pkappa = nullptr;
    double* d_ptsq = nullptr;
};

namespace {

BatchLinFeasOracle::Args batch_linfeas_args(const ellhip_batch_linfeas* o) {
    BatchLinFeasOracle::Args A;
    A.a = o->d_a;
    A.c = o->d_c;
    A.a_stride = o->shared ? 0 : (long long)o->J * o->n;
    A.c_stride = o->shared ? 0 : (long long)o->J;
    A.J = o->J;
    A.idx = o->d_idx;
    A.target = o->d_target;
    return A;
}

constexpr BatchLoopWords BATCH_LINFEAS_WORDS{"linfeas", "(n, J)", ""};

int batch_linfeas_feas(ellhip_batch* s, ellhip_batch_linfeas* o, int64_t max_iters, double tol, double* x_out,
                       int32_t* feasible_out, int64_t* niter_out, int32_t* status_out, BatchLoopEngine engine) {
    if (!s || !o || !feasible_out || !niter_out || !status_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_loop_run<BatchLinFeasOracle, BATCH_DRIVER_OPTIM, /*STREAMED=*/false>(
        s, o->loop, batch_linfeas_args(o), BATCH_LINFEAS_WORDS, engine, 1, nullptr, max_iters, tol, x_out, feasible_out,
        niter_out, status_out);
}

template <int T, bool STABLE>
int batch_bsearch_launch(const ellhip_batch* s, const BatchLoopShape& sh, size_t lds, const BatchBsRun& R,
                         const BatchBsBuffers& W, const BatchLinFeasOracle::Args& A, const EllCalcDev& calc) {
    if (const int rc = batch_loop_allow_lds<&k_batch_bsearch<T, STABLE, BatchLinFeasOracle>>(s->device, lds)) return rc;
    BatchParams P;
    P.B = s->B;
    P.n = s->n;
    P.pitch = batch_pitch(s->n);
    P.epw = sh.epw;
    P.K = 0;
    P.no_defer_trick = s->no_defer_trick;  // the clone honours it, as Clone does
    const unsigned grid = (unsigned)((s->B + sh.epw - 1) / sh.epw);
    hipLaunchKernelGGL((k_batch_bsearch<T, STABLE, BatchLinFeasOracle>), dim3(grid), dim3(T), lds, s->stream, P, R,
                       (const double*)s->d_Q, s->d_xc, (const double*)s->d_kappa, (const double*)s->d_tsq, W, A, calc);
    return 0;
}

// the probe buffers and the bisection state, on first use
hipError_t batch_bsearch_alloc(ellhip_batch_linfeas* o) {
    if (o->d_bs) return hipSuccess;
    const size_t B = (size_t)o->B, n = (size_t)o->n;
    double* bs = nullptr;
    hipError_t e = o->loop.mem.device(bs, B * BSS_N * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_bs_nstopped, sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_pQ, B * n * n * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_pxc, B * n * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_pkappa, B * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_ptsq, B * sizeof(double));
    if (e == hipSuccess) e = fill_now(o->d_pQ, 0, B * n * n * sizeof(double), o->loop.stream);
    if (e == hipSuccess) e = fill_now(o->d_pxc, 0, B * n * sizeof(double), o->loop.stream);
    if (e == hipSuccess) e = fill_now(o->d_pkappa, 0, B * sizeof(double), o->loop.stream);
    if (e == hipSuccess) e = fill_now(o->d_ptsq, 0, B * sizeof(double), o->loop.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->loop.stream);
    if (e == hipSuccess) o->d_bs = bs;  // (what was allocated before a failure stays with the handle's owner)
    return e;
}

// What every bsearch entry point checks before anything is touched: the handle's kind against the entry point's engine,
// B, n and the device, the iteration counts and the interval.
int batch_bsearch_check(const ellhip_batch* s, const ellhip_batch_linfeas* o, const double* lower, const double* upper,
                        int64_t inner_max_iters, int64_t max_iters, const int32_t* feasible_out, const int64_t* niter_out,
                        const double* upper_out, const int64_t* rounds_out, BatchLoopEngine engine, const std::string& what) {
    if (!s || !o || !lower || !upper || !feasible_out || !niter_out || !upper_out || !rounds_out)
        return fail(ELLHIP_E_INVALID, "NULL argument");
    if (!engine.streamed && s->streamed)
        return fail(ELLHIP_E_INVALID, (what + ": streamed batch handles are not supported: the LDS engines' kernel is not built "
                                              "for streamed handles; use ellhip_batch_linfeas_bsearch_streamed").c_str());
    if (const int rc = batch_loop_check(s, engine, what)) return rc;
    if (s->B != o->B || s->n != o->n) return fail(ELLHIP_E_INVALID, (what + ": spaces and oracle differ in B or n").c_str());
    if (s->device != o->loop.device)
        return fail(ELLHIP_E_INVALID, (what + ": spaces and oracle live on different devices").c_str());
    if (max_iters < 0 || inner_max_iters < 0) return fail(ELLHIP_E_INVALID, "max_iters and inner_max_iters must be >= 0");
    for (long long b = 0; b < o->B; ++b)
        if (!(lower[b] <= upper[b]))  // the reference asserts                                     src/cutting_plane.rs:448
            return fail(ELLHIP_E_INVALID, (what + ": lower > upper").c_str());
    return 0;
}

// The host loop of every bsearch kernel.  The caller has checked its arguments (batch_bsearch_check, the LDS a launch
// needs).  stride: the doubles of the kernel's state record, BS_N or BSS_N; launch(R, W) enqueues one launch of R.iters
// rounds on s->stream and returns 0 or an error code.
template <class Launch>
int batch_bsearch_drive(ellhip_batch* s, ellhip_batch_linfeas* o, const double* lower, const double* upper,
                        int64_t inner_max_iters, double inner_tol, int64_t max_iters, double tol, int32_t* feasible_out,
                        int64_t* niter_out, double* upper_out, int64_t* rounds_out, int64_t* ends_out, int stride,
                        Launch launch) {
    const size_t B = (size_t)o->B, N = (size_t)stride;
    DeviceGuard guard(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    {
        const hipError_t e = batch_bsearch_alloc(o);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched bsearch allocation", e);
    }
    std::vector<double> st(B * N, 0.0);
    for (size_t b = 0; b < B; ++b) {
        double* v = st.data() + b * N;
        v[BS_LOWER] = lower[b];
        v[BS_UPPER] = upper[b];
        v[BS_UORIG] = upper[b];  //                                                                                :449
        v[BS_INNER] = -1.0;      // between two probes
    }
    HIPCHK(hipMemcpy(o->d_bs, st.data(), B * N * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(fill_now(o->d_bs_nstopped, 0, sizeof(int), s->stream));
    BatchBsBuffers W;
    W.state = o->d_bs;
    W.nstopped = o->d_bs_nstopped;
    W.Q = o->d_pQ;
    W.xc = o->d_pxc;
    W.kappa = o->d_pkappa;
    W.tsq = o->d_ptsq;
    BatchBsRun R;
    R.iters = o->loop.chunk;
    R.inner_max_iters = inner_max_iters;
    R.inner_tol = inner_tol;
    R.max_iters = max_iters;
    R.tol = tol;
    // A launch runs `chunk` rounds of every instance that has not stopped; an instance needs at most
    // max_iters * inner_max_iters of them, and one launch when no probe makes an oracle call.
    const long double need = (long double)max_iters * ((long double)inner_max_iters + 1.0L);
    const long double cap = std::ceil(need / (long double)o->loop.chunk);
    const long long launches = std::max<long long>(1, cap > 4.0e18L ? (long long)4000000000000000000LL : (long long)cap);
    for (long long l = 0; l < launches; ++l) {
        if (const int rc = launch(R, W)) return rc;
        HIPCHK(hipGetLastError());
        int nstopped = 0;
        HIPCHK(hipMemcpyAsync(&nstopped, o->d_bs_nstopped, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        if ((long long)nstopped >= o->B) break;
    }
    HIPCHK(hipMemcpy(st.data(), o->d_bs, B * N * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        const double* v = st.data() + b * N;
        feasible_out[b] = v[BS_UPPER] != v[BS_UORIG];  //                                                     :454 / :465
        niter_out[b] = (int64_t)v[BS_NITER];
        upper_out[b] = v[BS_UPPER];
        rounds_out[b] = (int64_t)v[BS_ROUNDS];
        if (ends_out)
            for (int k = 0; k < 4; ++k) ends_out[4 * b + k] = (int64_t)v[BS_END + k];
    }
    return 0;
}

int batch_linfeas_bsearch(ellhip_batch* s, ellhip_batch_linfeas* o, const double* lower, const double* upper,
                          int64_t inner_max_iters, double inner_tol, int64_t max_iters, double tol, int32_t* feasible_out,
                          int64_t* niter_out, double* upper_out, int64_t* rounds_out, int64_t* ends_out,
                          BatchLoopEngine engine) {
    const std::string what = "batched bsearch";
    if (const int rc = batch_bsearch_check(s, o, lower, upper, inner_max_iters, max_iters, feasible_out, niter_out, upper_out,
                                           rounds_out, engine, what))
        return rc;
    const BatchLinFeasOracle::Args A = batch_linfeas_args(o);
    const BatchLoopShape sh = batch_loop_shape(s, engine.stable);
    const size_t lds =
        (size_t)sh.epw * (sh.space_doubles + BatchLinFeasOracle::lds_doubles(A, s->n) + BS_N) * sizeof(double);
    if (lds > BATCH_LOOP_LDS_MAX)
        return fail(ELLHIP_E_INVALID, (what + ": this (n, J) needs more LDS than a workgroup has").c_str());
    const EllCalcDev calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    return batch_bsearch_drive(s, o, lower, upper, inner_max_iters, inner_tol, max_iters, tol, feasible_out, niter_out,
                               upper_out, rounds_out, ends_out, BS_N, [&](const BatchBsRun& R, const BatchBsBuffers& W) {
        if (engine.stable)
            return sh.T == 128 ? batch_bsearch_launch<128, true>(s, sh, lds, R, W, A, calc)
                               : batch_bsearch_launch<256, true>(s, sh, lds, R, W, A, calc);
        return sh.T == 64    ? batch_bsearch_launch<64, false>(s, sh, lds, R, W, A, calc)
               : sh.T == 128 ? batch_bsearch_launch<128, false>(s, sh, lds, R, W, A, calc)
                             : batch_bsearch_launch<256, false>(s, sh, lds, R, W, A, calc);
    });
}

// ellhip_batch_linfeas_create and _create_streamed: the limits are the entry point's
int batch_linfeas_create(ellhip_batch_linfeas** out, int64_t B, int64_t n, int64_t J, const double* a, const double* c,
                         int32_t shared, int device, int nmax, int jmax) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1 || B > (1 << 24)) return fail(ELLHIP_E_INVALID, "batched linfeas: need 1 <= B <= 2^24");
    if (n < 1 || n > nmax) return fail(ELLHIP_E_INVALID, ("batched linfeas: need 1 <= n <= " + std::to_string(nmax)).c_str());
    if (J < 1 || J > jmax) return fail(ELLHIP_E_INVALID, ("batched linfeas: need 1 <= J <= " + std::to_string(jmax)).c_str());
    if (!a || !c) return fail(ELLHIP_E_INVALID, "NULL argument");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched linfeas oracle has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_batch_linfeas* o = new (std::nothrow) ellhip_batch_linfeas();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->B = B;
    o->n = (int)n;
    o->J = (int)J;
    o->shared = shared != 0;
    DeviceGuard guard(device);
    auto bail = [&](int code) {
        ellhip_batch_linfeas_destroy(o);
        return code;
    };
    const size_t sB = (size_t)B, sn = (size_t)n, sJ = (size_t)J;
    const size_t tables = o->shared ? 1 : sB;
    hipError_t e = batch_loop_alloc(o->loop, device, B, (int)n);
    if (e == hipSuccess) e = o->loop.mem.device(o->d_a, tables * sJ * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_c, tables * sJ * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_idx, sB * sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_target, sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_x, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_grad, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_beta, sB * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_cut, sB * sizeof(int));
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched linfeas allocation", e));
    const std::vector<double> target(sB, -1e100);  //                                                src/example3.rs:16
    e = fill_now(o->d_idx, 0xff, sB * sizeof(int), o->loop.stream);  // idx = -1                                   :15
    if (e == hipSuccess) e = hipMemcpy(o->d_target, target.data(), sB * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_a, a, tables * sJ * sn * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_c, c, tables * sJ * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched linfeas upload", e));
    *out = o;
    return 0;
}

}  // namespace

extern "C" {

int ellhip_batch_linfeas_create(ellhip_batch_linfeas** out, int64_t B, int64_t n, int64_t J, const double* a,
                                const double* c, int32_t shared, int device) {
    return batch_linfeas_create(out, B, n, J, a, c, shared, device, BATCH_NMAX, BATCH_LINFEAS_JMAX);
}

void ellhip_batch_linfeas_destroy(ellhip_batch_linfeas* o) {
    if (!o) return;
    DeviceGuard guard(o->loop.device);
    batch_loop_free(o->loop);
    delete o;
}

int ellhip_batch_linfeas_set_chunk(ellhip_batch_linfeas* o, int64_t iters) {
    return batch_loop_set_chunk(o ? &o->loop : nullptr, iters, "batched linfeas");
}

int ellhip_batch_linfeas_set_target(ellhip_batch_linfeas* o, const double* gamma) {
    if (!o || !gamma) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->loop.device);
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(o->d_target, gamma, (size_t)o->B * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

int ellhip_batch_linfeas_state(ellhip_batch_linfeas* o, int32_t* idx_out, double* target_out) {
    if (!o || !idx_out || !target_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    static_assert(sizeof(int) == sizeof(int32_t), "the cursors are copied as they are");
    DeviceGuard guard(o->loop.device);
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(idx_out, o->d_idx, (size_t)o->B * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(target_out, o->d_target, (size_t)o->B * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int ellhip_batch_linfeas_assess_feas(ellhip_batch_linfeas* o, const double* x, double* grad_out, double* beta_out,
                                     int32_t* cut_out) {
    if (!o || !x || !grad_out || !beta_out || !cut_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->loop.device);
    const size_t B = (size_t)o->B, n = (size_t)o->n;
    const BatchLinFeasOracle::Args A = batch_linfeas_args(o);
    const size_t per = BatchLinFeasOracle::lds_doubles(A, o->n) + n;
    const bool wide = o->n > BATCH_NMAX;  // past the LDS engines' block: one workgroup per problem, n rounded up to whole waves
    const BatchRowShape sh = wide ? BatchRowShape{} : batch_row_shape(o->n, per);  // (epw = 1 when wide)
    const size_t lds = (size_t)sh.epw * per * sizeof(double);
    const unsigned grid = (unsigned)((o->B + sh.epw - 1) / sh.epw);
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(o->d_x, x, B * n * sizeof(double), hipMemcpyHostToDevice));
    if (wide)
        hipLaunchKernelGGL(k_batch_linfeas_assess_wg, dim3(grid), dim3((unsigned)((o->n + 63) / 64 * 64)), lds, o->loop.stream,
                           o->n, A, (const double*)o->d_x, o->d_grad, o->d_beta, o->d_cut);
    else if (sh.T == 128)
        hipLaunchKernelGGL(k_batch_linfeas_assess<128>, dim3(grid), dim3(128), lds, o->loop.stream, o->B, o->n, sh.epw, A,
                           (const double*)o->d_x, o->d_grad, o->d_beta, o->d_cut);
    else
        hipLaunchKernelGGL(k_batch_linfeas_assess<256>, dim3(grid), dim3(256), lds, o->loop.stream, o->B, o->n, sh.epw, A,
                           (const double*)o->d_x, o->d_grad, o->d_beta, o->d_cut);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(grad_out, o->d_grad, B * n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(beta_out, o->d_beta, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cut_out, o->d_cut, B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int ellhip_batch_linfeas_feas(ellhip_batch* spaces, ellhip_batch_linfeas* o, int64_t max_iters, double tol, double* x_out,
                              int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_linfeas_feas(spaces, o, max_iters, tol, x_out, feasible_out, niter_out, status_out, BATCH_ENGINE_LDS);
}

int ellhip_batch_linfeas_feas_stable(ellhip_batch* spaces, ellhip_batch_linfeas* o, int64_t max_iters, double tol,
                                     double* x_out, int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_linfeas_feas(spaces, o, max_iters, tol, x_out, feasible_out, niter_out, status_out, BATCH_ENGINE_LDS_STABLE);
}

int ellhip_batch_linfeas_bsearch(ellhip_batch* spaces, ellhip_batch_linfeas* o, const double* lower, const double* upper,
                                 int64_t inner_max_iters, double inner_tol, int64_t max_iters, double tol,
                                 int32_t* feasible_out, int64_t* niter_out, double* upper_out, int64_t* rounds_out,
                                 int64_t* ends_out) {
    return batch_linfeas_bsearch(spaces, o, lower, upper, inner_max_iters, inner_tol, max_iters, tol, feasible_out, niter_out,
                                 upper_out, rounds_out, ends_out, BATCH_ENGINE_LDS);
}

int ellhip_batch_linfeas_bsearch_stable(ellhip_batch* spaces, ellhip_batch_linfeas* o, const double* lower,
                                        const double* upper, int64_t inner_max_iters, double inner_tol, int64_t max_iters,
                                        double tol, int32_t* feasible_out, int64_t* niter_out, double* upper_out,
                                        int64_t* rounds_out, int64_t* ends_out) {
    return batch_linfeas_bsearch(spaces, o, lower, upper, inner_max_iters, inner_tol, max_iters, tol, feasible_out, niter_out,
                                 upper_out, rounds_out, ends_out, BATCH_ENGINE_LDS_STABLE);
}

}  // extern "C"
