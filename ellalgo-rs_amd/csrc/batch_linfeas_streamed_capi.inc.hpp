// batch_linfeas_streamed_capi.inc.hpp -- C ABI of the batched linear feasibility loops and of the device-resident bsearch on
// streamed batch handles, Ell and EllStable (include/ellhip_batch_bsearch_streamed.h).  Included at the
// end of ellhip_capi.hip, after batch_linfeas_capi.inc.hpp: the oracle handle, the constructor (batch_linfeas_create), the
// argument checks (batch_bsearch_check) and the host loop (batch_bsearch_drive) are that file's.
//
// The _feas entry points are two more engines of batch_loop_run (k_batch_streamed_loop<BatchLinFeasOracle> and
// k_batch_streamed_loop_stable<BatchLinFeasOracle>); the _bsearch ones launch k_batch_streamed_bsearch and
// k_batch_streamed_bsearch_stable of batch_linfeas_streamed_kernels.hpp.
//
// Reference: src/example3.rs (oracle), src/cutting_plane.rs:205-227 (cutting_plane_feas), :403-419 (BSearchAdaptor),
// :441-466 (bsearch).
#include "../../include/ellhip_batch_bsearch_streamed.h"

#include "batch_linfeas_streamed_kernels.hpp"

static_assert(ELLHIP_BATCH_LINFEAS_STREAMED_JMAX == ellhip::BATCH_LINFEAS_STREAMED_JMAX, "header and kernel disagree on J");

namespace {

int batch_linfeas_feas_streamed(ellhip_batch* s, ellhip_batch_linfeas* o, int64_t max_iters, double tol, double* x_out,
                                int32_t* feasible_out, int64_t* niter_out, int32_t* status_out, BatchLoopEngine engine) {
    if (!s || !o || !feasible_out || !niter_out || !status_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_loop_run<BatchLinFeasOracle, BATCH_DRIVER_OPTIM, /*STREAMED=*/true>(
        s, o->loop, batch_linfeas_args(o), BATCH_LINFEAS_WORDS, engine, 1, nullptr, max_iters, tol, x_out, feasible_out,
        niter_out, status_out);
}

// one workgroup per problem, the block the streamed handle was shaped with
template <bool STABLE>
int batch_streamed_bsearch_launch(const ellhip_batch* s, size_t lds, const BatchBsRun& R, const BatchBsBuffers& W,
                                  const BatchLinFeasOracle::Args& A, const EllCalcDev& calc) {
    BatchStreamedParams P;
    P.B = s->B;
    P.n = s->n;
    P.np = batch_streamed_np(s->n);
    P.K = 0;
    P.no_defer_trick = STABLE ? 0 : s->no_defer_trick;  // Ell only: the clone honours it, as Clone does
    if constexpr (STABLE) {
        if (const int rc = batch_loop_allow_lds<&k_batch_streamed_bsearch_stable<BatchLinFeasOracle>>(s->device, lds)) return rc;
        hipLaunchKernelGGL(k_batch_streamed_bsearch_stable<BatchLinFeasOracle>, dim3((unsigned)s->B), dim3(s->T), lds, s->stream,
                           P, R, (const double*)s->d_Q, s->d_xc, (const double*)s->d_kappa, (const double*)s->d_tsq, W, A, calc);
    } else {
        if (const int rc = batch_loop_allow_lds<&k_batch_streamed_bsearch<BatchLinFeasOracle>>(s->device, lds)) return rc;
        hipLaunchKernelGGL(k_batch_streamed_bsearch<BatchLinFeasOracle>, dim3((unsigned)s->B), dim3(s->T), lds, s->stream, P, R,
                           (const double*)s->d_Q, s->d_xc, (const double*)s->d_kappa, (const double*)s->d_tsq,
                           (const int*)s->d_sym, W, A, calc);
    }
    return 0;
}

int batch_linfeas_bsearch_streamed(ellhip_batch* s, ellhip_batch_linfeas* o, const double* lower, const double* upper,
                                   int64_t inner_max_iters, double inner_tol, int64_t max_iters, double tol,
                                   int32_t* feasible_out, int64_t* niter_out, double* upper_out, int64_t* rounds_out,
                                   int64_t* ends_out, BatchLoopEngine engine) {
    const std::string what = engine.stable ? "batched streamed EllStable bsearch" : "batched streamed bsearch";
    if (const int rc = batch_bsearch_check(s, o, lower, upper, inner_max_iters, max_iters, feasible_out, niter_out, upper_out,
                                           rounds_out, engine, what))
        return rc;
    const BatchLinFeasOracle::Args A = batch_linfeas_args(o);
    const size_t lds = batch_streamed_bsearch_lds_doubles<BatchLinFeasOracle>(A, s->n, engine.stable) * sizeof(double);
    if (lds > BATCH_LOOP_LDS_MAX)
        return fail(ELLHIP_E_INVALID, (what + ": this (n, J) needs more LDS than a workgroup has").c_str());
    const EllCalcDev calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    return batch_bsearch_drive(s, o, lower, upper, inner_max_iters, inner_tol, max_iters, tol, feasible_out, niter_out,
                               upper_out, rounds_out, ends_out, BSS_N, [&](const BatchBsRun& R, const BatchBsBuffers& W) {
        return engine.stable ? batch_streamed_bsearch_launch<true>(s, lds, R, W, A, calc)
                             : batch_streamed_bsearch_launch<false>(s, lds, R, W, A, calc);
    });
}

}  // namespace

extern "C" {

int ellhip_batch_linfeas_create_streamed(ellhip_batch_linfeas** out, int64_t B, int64_t n, int64_t J, const double* a,
                                         const double* c, int32_t shared, int device) {
    return batch_linfeas_create(out, B, n, J, a, c, shared, device, BATCH_STREAMED_NMAX, BATCH_LINFEAS_STREAMED_JMAX);
}

int ellhip_batch_linfeas_feas_streamed(ellhip_batch* spaces, ellhip_batch_linfeas* o, int64_t max_iters, double tol,
                                       double* x_out, int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_linfeas_feas_streamed(spaces, o, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                                       BATCH_ENGINE_STREAMED);
}

int ellhip_batch_linfeas_feas_streamed_stable(ellhip_batch* spaces, ellhip_batch_linfeas* o, int64_t max_iters, double tol,
                                              double* x_out, int32_t* feasible_out, int64_t* niter_out,
                                              int32_t* status_out) {
    return batch_linfeas_feas_streamed(spaces, o, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                                       BATCH_ENGINE_STREAMED_STABLE);
}

int ellhip_batch_linfeas_bsearch_streamed(ellhip_batch* spaces, ellhip_batch_linfeas* o, const double* lower,
                                          const double* upper, int64_t inner_max_iters, double inner_tol, int64_t max_iters,
                                          double tol, int32_t* feasible_out, int64_t* niter_out, double* upper_out,
                                          int64_t* rounds_out, int64_t* ends_out) {
    return batch_linfeas_bsearch_streamed(spaces, o, lower, upper, inner_max_iters, inner_tol, max_iters, tol, feasible_out,
                                          niter_out, upper_out, rounds_out, ends_out, BATCH_ENGINE_STREAMED);
}

int ellhip_batch_linfeas_bsearch_streamed_stable(ellhip_batch* spaces, ellhip_batch_linfeas* o, const double* lower,
                                                 const double* upper, int64_t inner_max_iters, double inner_tol,
                                                 int64_t max_iters, double tol, int32_t* feasible_out, int64_t* niter_out,
                                                 double* upper_out, int64_t* rounds_out, int64_t* ends_out) {
    return batch_linfeas_bsearch_streamed(spaces, o, lower, upper, inner_max_iters, inner_tol, max_iters, tol, feasible_out,
                                          niter_out, upper_out, rounds_out, ends_out, BATCH_ENGINE_STREAMED_STABLE);
}

}  // extern "C"
