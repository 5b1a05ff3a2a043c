// batch_loop_capi.inc.hpp -- the host side the batched device-resident cutting-plane loops share: the loop state an oracle
// handle owns, the launch shapes and the one driver that runs the loop kernel of a batch engine -- k_batch_loop
// (batch_loop_kernels.hpp) on the LDS engine, k_batch_streamed_loop (batch_streamed_loop_kernels.hpp) and
// k_batch_streamed_loop_stable (batch_streamed_stable_loop_kernels.hpp) on the streamed one -- over a batch handle.
// Included at the end of ellhip_capi.hip, after batch_capi.inc.hpp, batch_streamed_capi.inc.hpp and
// batch_streamed_stable_capi.inc.hpp (it drives the batch engines' handle directly) and before every batch_*_capi.inc.hpp
// of an oracle.
//
// Reference: src/cutting_plane.rs:205-227, 286-313, 331-374 (loops).
#include "batch_loop_kernels.hpp"
#include "batch_streamed_loop_kernels.hpp"
#include "batch_streamed_stable_loop_kernels.hpp"

namespace {

// The part of an oracle handle that every batched loop has: where the handle lives, its stream, the loop state, and the
// owner of ALL the handle's device memory (the oracle's own buffers too: one release in batch_loop_free).
struct BatchLoopBuffers {
    Allocs mem;
    int device = 0;
    long long B = 0;
    int n = 0;
    int chunk = 256;               // iterations per launch
    double* d_gamma = nullptr;     // [B]
    double* d_xbest = nullptr;     // [B][n]
    long long* d_niter = nullptr;  // [B]
    int* d_ints = nullptr;         // has_best [B], stopped [B], status [B], nstopped [1]
    hipStream_t stream = nullptr;
};

// the stream and the buffers, zeroed
hipError_t batch_loop_alloc(BatchLoopBuffers& st, int device, long long B, int n) {
    st.device = device;
    st.B = B;
    st.n = n;
    const size_t sB = (size_t)B, sn = (size_t)n;
    hipError_t e = hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = st.mem.device(st.d_gamma, sB * sizeof(double));
    if (e == hipSuccess) e = st.mem.device(st.d_xbest, sB * sn * sizeof(double));
    if (e == hipSuccess) e = st.mem.device(st.d_niter, sB * sizeof(long long));
    if (e == hipSuccess) e = st.mem.device(st.d_ints, (3 * sB + 1) * sizeof(int));
    if (e == hipSuccess) e = fill_now(st.d_gamma, 0, sB * sizeof(double), st.stream);
    if (e == hipSuccess) e = fill_now(st.d_xbest, 0, sB * sn * sizeof(double), st.stream);
    if (e == hipSuccess) e = fill_now(st.d_niter, 0, sB * sizeof(long long), st.stream);
    if (e == hipSuccess) e = fill_now(st.d_ints, 0, (3 * sB + 1) * sizeof(int), st.stream);
    return e;
}

// a new solve: nobody has stopped, nobody has a best point, no iteration done (x_best rows are only read where has_best)
hipError_t batch_loop_reset(BatchLoopBuffers& st, hipStream_t stream) {
    const size_t sB = (size_t)st.B;
    const hipError_t e = fill_now(st.d_ints, 0, (3 * sB + 1) * sizeof(int), stream);
    return e == hipSuccess ? fill_now(st.d_niter, 0, sB * sizeof(long long), stream) : e;
}

// waits for the stream, releases the handle's memory, then the stream; the caller has selected the device
void batch_loop_free(BatchLoopBuffers& st) {
    if (st.stream) (void)hipStreamSynchronize(st.stream);
    st.mem.release_all();
    if (st.stream) (void)hipStreamDestroy(st.stream);
    st.stream = nullptr;
}

BatchLoopState batch_loop_view(const BatchLoopBuffers& st) {
    const size_t sB = (size_t)st.B;
    BatchLoopState S;
    S.gamma = st.d_gamma;
    S.xbest = st.d_xbest;
    S.has_best = st.d_ints;
    S.niter = st.d_niter;
    S.stopped = st.d_ints + sB;
    S.status = st.d_ints + 2 * sB;
    S.nstopped = st.d_ints + 3 * sB;
    return S;
}

int batch_loop_set_chunk(BatchLoopBuffers* st, int64_t iters, const char* what) {
    if (!st) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (iters < 1 || iters > 4096) return fail(ELLHIP_E_INVALID, (std::string(what) + ": chunk must be in 1..4096").c_str());
    st->chunk = (int)iters;
    return 0;
}

// 160 KiB per workgroup, less the 1 KiB kept for the kernel's static LDS (the barrier votes)
constexpr size_t BATCH_LOOP_LDS_MAX = 159 * 1024;

// More than the default 64 KiB of dynamic LDS needs an opt-in per kernel and per device; a launch within 64 KiB needs none
// and never comes past the first line.  As in batch_shape it is only ever raised; the high-water marks are the kernel's own
// (one instantiation of this function, and so one table, per kernel instantiation).
template <auto Kernel>
int batch_loop_allow_lds(int device, size_t bytes) {
    constexpr int MAXDEV = 64;
    static std::atomic<int> granted[MAXDEV];
    if (bytes <= 64 * 1024) return 0;
    const bool known = device >= 0 && device < MAXDEV;
    if (known && (int)bytes <= granted[device].load()) return 0;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (known) {
        int seen = granted[device].load();
        while (seen < (int)bytes && !granted[device].compare_exchange_weak(seen, (int)bytes)) {}
    }
    return 0;
}

// n threads per instance without a batch handle's own shape: 256 threads up to n = 64, else 128; at most 64 instances
// (one wave runs the scalar stage, one lane per instance) and at most 64 KiB of `doubles` per instance
struct BatchRowShape {
    int T = 64, epw = 1;
};
BatchRowShape batch_row_shape(int n, size_t doubles) {
    BatchRowShape r;
    r.T = n <= 64 ? 256 : 128;
    r.epw = std::min(64, r.T / n);
    while (r.epw > 1 && (size_t)r.epw * doubles * sizeof(double) > 64 * 1024) r.epw -= 1;
    return r;
}

// How k_batch_loop is launched on a batch handle of the LDS engine.  An Ell handle is launched as the batch engine shaped
// it.  An EllStable handle is shaped for k_batch_update_stable's one lane per ellipsoid (one wave, up to 64 ellipsoids); the
// loop kernel gives an instance n threads, so it takes batch_row_shape with batch_stable_apply_lds_doubles in it.
struct BatchLoopShape {
    int T = 64, epw = 1;
    size_t space_doubles = 0;  // LDS doubles of one instance's space
};

BatchLoopShape batch_loop_shape(const ellhip_batch* s, bool stable) {
    BatchLoopShape sh;
    if (!stable) {
        sh.T = s->T;
        sh.epw = s->epw;
        sh.space_doubles = batch_lds_doubles(s->n);
    } else {
        sh.space_doubles = batch_stable_apply_lds_doubles(s->n);
        const BatchRowShape r = batch_row_shape(s->n, sh.space_doubles);
        sh.T = r.T;
        sh.epw = r.epw;
    }
    return sh;
}

// The engine an entry point runs on: the LDS engine (include/ellhip_batch.h) or the streamed one
// (include/ellhip_batch_streamed.h), with Ell or with EllStable spaces.  The plain entry points are {false, false}; the
// suffixes _stable, _streamed and _streamed_stable name the other three.
struct BatchLoopEngine {
    bool streamed, stable;
};
constexpr BatchLoopEngine BATCH_ENGINE_LDS{false, false}, BATCH_ENGINE_LDS_STABLE{false, true},
    BATCH_ENGINE_STREAMED{true, false}, BATCH_ENGINE_STREAMED_STABLE{true, true};

// What a refusal calls the oracle, the shape and the dimension; what it calls the loop comes from the engine.
struct BatchLoopWords {
    const char* oracle;  // "LMI"
    const char* shape;   // "(n, m)": what decides the LDS an instance needs
    const char* n_is;    // "" or how the oracle's n comes about
};

// "batched LMI loop" on both LDS engines (the _stable entry points share the plain ones' words), "batched LMI streamed loop",
// "batched LMI streamed EllStable loop"
std::string batch_loop_what(const char* oracle, BatchLoopEngine e) {
    return std::string("batched ") + oracle + (!e.streamed ? " loop" : e.stable ? " streamed EllStable loop" : " streamed loop");
}

// the handle's kind against the entry point's engine: first the engine (a streamed handle keeps its matrices in HBM, the LDS
// engine's kernel keeps them in LDS), then the variant
int batch_loop_check(const ellhip_batch* s, BatchLoopEngine e, const std::string& what) {
    const std::string entry =
        std::string("the ") + (e.streamed ? "_streamed" : "") + (e.stable ? "_stable" : "") + " entry points take ";
    if (e.streamed && !s->streamed) return fail(ELLHIP_E_INVALID, (what + ": " + entry + "streamed batch handles only").c_str());
    if (!e.streamed && s->streamed) return fail(ELLHIP_E_INVALID, (what + ": streamed batch handles are not supported").c_str());
    if (s->variant == (e.stable ? ELLHIP_SPACE_ELL_STABLE : ELLHIP_SPACE_ELL)) return 0;
    return fail(ELLHIP_E_INVALID, (what + ": " + (e.stable ? entry + "EllStable batch handles only"
                                                          : "EllStable batch handles are not supported")).c_str());
}

template <int T, bool STABLE, class Oracle, int DRIVER = BATCH_DRIVER_OPTIM>
int batch_loop_launch(const ellhip_batch* s, const BatchLoopShape& sh, size_t lds, const BatchLoopRun& R,
                      const BatchLoopState& S, const typename Oracle::Args& A, const EllCalcDev& calc) {
    if (const int rc = batch_loop_allow_lds<&k_batch_loop<T, STABLE, Oracle, DRIVER>>(s->device, lds)) return rc;
    BatchParams P;
    P.B = s->B;
    P.n = s->n;
    P.pitch = batch_pitch(s->n);
    P.epw = sh.epw;
    P.K = 0;
    P.no_defer_trick = s->no_defer_trick;
    const unsigned grid = (unsigned)((s->B + sh.epw - 1) / sh.epw);
    hipLaunchKernelGGL((k_batch_loop<T, STABLE, Oracle, DRIVER>), dim3(grid), dim3(T), lds, s->stream, P, R, s->d_Q, s->d_xc,
                       s->d_kappa, s->d_tsq, S, A, calc);
    return 0;
}

// one workgroup per instance, the block the streamed handle was shaped with
template <bool STABLE, class Oracle>
int batch_streamed_loop_launch(const ellhip_batch* s, size_t lds, const BatchLoopRun& R, const BatchLoopState& S,
                               const typename Oracle::Args& A, const EllCalcDev& calc) {
    BatchStreamedParams P;
    P.B = s->B;
    P.n = s->n;
    P.np = batch_streamed_np(s->n);
    P.K = 0;
    P.no_defer_trick = STABLE ? 0 : s->no_defer_trick;  // Ell only: the EllStable handle refuses the setter
    if constexpr (STABLE) {
        if (const int rc = batch_loop_allow_lds<&k_batch_streamed_loop_stable<Oracle>>(s->device, lds)) return rc;
        hipLaunchKernelGGL(k_batch_streamed_loop_stable<Oracle>, dim3((unsigned)s->B), dim3(s->T), lds, s->stream, P, R, s->d_Q,
                           s->d_xc, s->d_kappa, s->d_tsq, S, A, calc);
    } else {
        if (const int rc = batch_loop_allow_lds<&k_batch_streamed_loop<Oracle>>(s->device, lds)) return rc;
        hipLaunchKernelGGL(k_batch_streamed_loop<Oracle>, dim3((unsigned)s->B), dim3(s->T), lds, s->stream, P, R, s->d_Q, s->d_xc,
                           s->d_kappa, s->d_tsq, s->d_sym, S, A, calc);
    }
    return 0;
}

// The part of a run that does not depend on the kernel: cutting_plane_optim (feas = 0, gamma in and out) or
// cutting_plane_feas for every instance, up to max_iters rounds in launches of st.chunk until every instance has stopped,
// then the results.  launch(R) enqueues one launch of R.iters rounds on s->stream and returns 0 or an error code.  The
// caller has checked that the spaces and the oracle fit each other.  d_retry: the optim_q driver's retry flags [B], part of
// the oracle's state in HBM and false when a run begins (src/cutting_plane.rs:343); null for the other drivers.
template <class Launch>
int batch_loop_drive(ellhip_batch* s, BatchLoopBuffers& st, int feas, double* gamma_inout, int64_t max_iters, double tol,
                     double* x_out, int32_t* has_out, int64_t* niter_out, int32_t* status_out, int* d_retry, Launch launch) {
    if (max_iters < 0) return fail(ELLHIP_E_INVALID, "max_iters must be >= 0");
    const size_t B = (size_t)st.B, n = (size_t)st.n;
    DeviceGuard guard(s->device);
    const BatchLoopState S = batch_loop_view(st);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipStreamSynchronize(st.stream));
    HIPCHK(batch_loop_reset(st, s->stream));
    if (d_retry) HIPCHK(fill_now(d_retry, 0, B * sizeof(int), s->stream));
    if (!feas) HIPCHK(hipMemcpy(st.d_gamma, gamma_inout, B * sizeof(double), hipMemcpyHostToDevice));
    BatchLoopRun R;
    R.feas = feas;
    R.max_iters = max_iters;
    R.tol = tol;
    for (long long done = 0; done < max_iters; done += st.chunk) {
        R.iters = (int)std::min<long long>(st.chunk, max_iters - done);
        if (const int rc = launch(R)) return rc;
        HIPCHK(hipGetLastError());
        int nstopped = 0;
        HIPCHK(hipMemcpyAsync(&nstopped, S.nstopped, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        if ((long long)nstopped >= st.B) break;
    }
    std::vector<int32_t> has(B);
    std::vector<long long> niter(B);
    HIPCHK(hipMemcpy(has.data(), S.has_best, B * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status_out, S.status, B * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(niter.data(), st.d_niter, B * sizeof(long long), hipMemcpyDeviceToHost));
    if (!feas) HIPCHK(hipMemcpy(gamma_inout, st.d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        has_out[b] = has[b];
        niter_out[b] = niter[b];
    }
    if (x_out) {
        std::vector<double> xb(B * n);
        HIPCHK(hipMemcpy(xb.data(), st.d_xbest, B * n * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b)
            if (has[b]) memcpy(x_out + b * n, xb.data() + b * n, n * sizeof(double));
    }
    return 0;
}

// The loops of one oracle on one engine: the loop kernel of `engine` over a batch handle of that engine's kind.  The caller
// has checked its pointers.  DRIVER: which of the reference's drivers (batch_loop_kernels.hpp); the optim_q driver takes the
// oracle's retry flags in d_retry.  STREAMED = false: an oracle that has the LDS engines' loop kernels only (the streamed
// ones are then not built for it, and a streamed engine is refused).
template <class Oracle, int DRIVER = BATCH_DRIVER_OPTIM, bool STREAMED = true>
int batch_loop_run(ellhip_batch* s, BatchLoopBuffers& st, const typename Oracle::Args& A, const BatchLoopWords& w,
                   BatchLoopEngine engine, int feas, double* gamma_inout, int64_t max_iters, double tol, double* x_out,
                   int32_t* has_out, int64_t* niter_out, int32_t* status_out, int* d_retry = nullptr) {
    static_assert(DRIVER == BATCH_DRIVER_OPTIM || !STREAMED, "the streamed loop kernels have no optim_q driver");
    const std::string what = batch_loop_what(w.oracle, engine);
    if (!STREAMED && engine.streamed) return fail(ELLHIP_E_INVALID, (what + ": there is no streamed form of this loop").c_str());
    if (const int rc = batch_loop_check(s, engine, what)) return rc;
    if (s->B != st.B || s->n != st.n)
        return fail(ELLHIP_E_INVALID, (what + ": spaces and oracle differ in B or n" + w.n_is).c_str());
    if (s->device != st.device) return fail(ELLHIP_E_INVALID, (what + ": spaces and oracle live on different devices").c_str());
    const BatchLoopShape sh = engine.streamed ? BatchLoopShape{} : batch_loop_shape(s, engine.stable);  // the LDS engine's
    size_t doubles = (size_t)sh.epw * (sh.space_doubles + Oracle::lds_doubles(A, s->n));
    if constexpr (STREAMED) {
        if (engine.streamed)
            doubles = engine.stable ? batch_streamed_stable_loop_lds_doubles<Oracle>(A, s->n)
                                    : batch_streamed_loop_lds_doubles<Oracle>(A, s->n);
    }
    const size_t lds = doubles * sizeof(double);
    if (lds > BATCH_LOOP_LDS_MAX)
        return fail(ELLHIP_E_INVALID, (what + ": this " + w.shape + " needs more LDS than a workgroup has").c_str());
    const EllCalcDev calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    const BatchLoopState S = batch_loop_view(st);
    return batch_loop_drive(s, st, feas, gamma_inout, max_iters, tol, x_out, has_out, niter_out, status_out, d_retry,
                            [&](const BatchLoopRun& R) {
        if constexpr (STREAMED) {
            if (engine.streamed)
                return engine.stable ? batch_streamed_loop_launch<true, Oracle>(s, lds, R, S, A, calc)
                                     : batch_streamed_loop_launch<false, Oracle>(s, lds, R, S, A, calc);
        }
        if (engine.stable)
            return sh.T == 128 ? batch_loop_launch<128, true, Oracle, DRIVER>(s, sh, lds, R, S, A, calc)
                               : batch_loop_launch<256, true, Oracle, DRIVER>(s, sh, lds, R, S, A, calc);
        return sh.T == 64    ? batch_loop_launch<64, false, Oracle, DRIVER>(s, sh, lds, R, S, A, calc)
               : sh.T == 128 ? batch_loop_launch<128, false, Oracle, DRIVER>(s, sh, lds, R, S, A, calc)
                             : batch_loop_launch<256, false, Oracle, DRIVER>(s, sh, lds, R, S, A, calc);
    });
}

}  // namespace
