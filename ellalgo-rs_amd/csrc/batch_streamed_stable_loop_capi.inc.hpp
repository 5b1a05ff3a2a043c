// batch_streamed_stable_loop_capi.inc.hpp -- C ABI of the batched device-resident low-pass design loop on a streamed EllStable
// batch handle (include/ellhip_batch_lowpass_streamed_stable.h).  Included at the end of ellhip_capi.hip, after
// batch_streamed_loop_capi.inc.hpp: the handle is batch_streamed_stable_capi.inc.hpp's, the loop state and batch_loop_drive
// are batch_loop_capi.inc.hpp's, the oracle handle is batch_lowpass_capi.inc.hpp's.
#include "../../include/ellhip_batch_lowpass_streamed_stable.h"

#include "batch_streamed_stable_loop_kernels.hpp"

namespace {

// The loops on the streamed engine's EllStable handles: k_batch_streamed_loop_stable.  The checks are
// batch_streamed_loop_run's with the variant test inverted.
template <class Oracle>
int batch_streamed_stable_loop_run(ellhip_batch* s, BatchLoopBuffers& st, const typename Oracle::Args& A,
                                   const BatchLoopWords& w, int feas, double* gamma_inout, int64_t max_iters, double tol,
                                   double* x_out, int32_t* has_out, int64_t* niter_out, int32_t* status_out) {
    const std::string what(w.what);
    if (!s->streamed)
        return fail(ELLHIP_E_INVALID, (what + ": the _streamed_stable entry points take streamed batch handles only").c_str());
    if (s->variant != ELLHIP_SPACE_ELL_STABLE)
        return fail(ELLHIP_E_INVALID, (what + ": the _streamed_stable entry points take EllStable batch handles only").c_str());
    if (s->B != st.B || s->n != st.n)
        return fail(ELLHIP_E_INVALID, (what + ": spaces and oracle differ in B or n" + w.n_is).c_str());
    if (s->device != st.device) return fail(ELLHIP_E_INVALID, (what + ": spaces and oracle live on different devices").c_str());
    const size_t lds = batch_streamed_stable_loop_lds_doubles<Oracle>(A, s->n) * sizeof(double);
    if (lds > BATCH_LOOP_LDS_MAX)
        return fail(ELLHIP_E_INVALID, (what + ": this " + w.shape + " needs more LDS than a workgroup has").c_str());
    BatchStreamedParams P;
    P.B = s->B;
    P.n = s->n;
    P.np = batch_streamed_np(s->n);
    P.K = 0;
    P.no_defer_trick = 0;  // Ell only: the handle refuses the setter
    const EllCalcDev calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    const BatchLoopState S = batch_loop_view(st);
    return batch_loop_drive(s, st, feas, gamma_inout, max_iters, tol, x_out, has_out, niter_out, status_out,
                            [&](const BatchLoopRun& R) {
        if (const int rc = batch_streamed_allow_lds<Oracle>(
                reinterpret_cast<const void*>(&k_batch_streamed_loop_stable<Oracle>), s->device, 1, lds))
            return rc;
        hipLaunchKernelGGL(k_batch_streamed_loop_stable<Oracle>, dim3((unsigned)s->B), dim3(s->T), lds, s->stream, P, R, s->d_Q,
                           s->d_xc, s->d_kappa, s->d_tsq, S, A, calc);
        return 0;
    });
}

int batch_lowpass_run_streamed_stable(ellhip_batch* s, ellhip_batch_lowpass* o, int feas, double* gamma_inout,
                                      int64_t max_iters, double tol, double* x_out, int32_t* has_out, int64_t* niter_out,
                                      int32_t* status_out) {
    if (!s || !o || !has_out || !niter_out || !status_out || (!feas && !gamma_inout))
        return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_streamed_stable_loop_run<BatchLpOracle>(s, o->loop, batch_lowpass_args(o),
                                                         {"batched lowpass streamed EllStable loop", "n", ""}, feas,
                                                         gamma_inout, max_iters, tol, x_out, has_out, niter_out, status_out);
}

}  // namespace

extern "C" {

int ellhip_batch_lowpass_optim_streamed_stable(ellhip_batch* spaces, ellhip_batch_lowpass* o, double* gamma_inout,
                                               int64_t max_iters, double tol, double* x_best_out, int32_t* has_best_out,
                                               int64_t* niter_out, int32_t* status_out) {
    return batch_lowpass_run_streamed_stable(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out,
                                             status_out);
}

int ellhip_batch_lowpass_feas_streamed_stable(ellhip_batch* spaces, ellhip_batch_lowpass* o, int64_t max_iters, double tol,
                                              double* x_out, int32_t* feasible_out, int64_t* niter_out,
                                              int32_t* status_out) {
    return batch_lowpass_run_streamed_stable(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out);
}

}  // extern "C"
