// batch_streamed_loop_capi.inc.hpp -- C ABI of the batched device-resident low-pass design loop on a streamed batch handle
// (include/ellhip_batch_lowpass_streamed.h).  Included at the end of ellhip_capi.hip, after batch_streamed_capi.inc.hpp (the
// handle), batch_loop_capi.inc.hpp (the loop state and batch_loop_drive) and batch_lowpass_capi.inc.hpp (the oracle handle).
#include "../../include/ellhip_batch_lowpass_streamed.h"

#include "batch_streamed_loop_kernels.hpp"

namespace {

// More than the default 64 KiB of dynamic LDS needs an opt-in per kernel and per device (batch_loop_allow_lds is the LDS
// driver's): raised only, once per (oracle, device, kernel), with the high-water marks kept here.  slot 0:
// k_batch_streamed_loop<Oracle>, slot 1: k_batch_streamed_loop_stable<Oracle>.  Launches within 64 KiB never come here, so
// the low-pass and SVM loops (at most 48.2 and 48.1 KiB) run as they did.
template <class Oracle>
int batch_streamed_allow_lds(const void* kernel, int device, int slot, size_t bytes) {
    constexpr int MAXDEV = 64;
    static std::atomic<int> granted[MAXDEV][2];
    if (bytes <= 64 * 1024) return 0;
    const bool known = device >= 0 && device < MAXDEV;
    if (known && (int)bytes <= granted[device][slot].load()) return 0;
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (known) {
        int seen = granted[device][slot].load();
        while (seen < (int)bytes && !granted[device][slot].compare_exchange_weak(seen, (int)bytes)) {}
    }
    return 0;
}

// The loops on the streamed engine: k_batch_streamed_loop over a streamed batch handle of Ell spaces.
template <class Oracle>
int batch_streamed_loop_run(ellhip_batch* s, BatchLoopBuffers& st, const typename Oracle::Args& A, const BatchLoopWords& w,
                            int feas, double* gamma_inout, int64_t max_iters, double tol, double* x_out, int32_t* has_out,
                            int64_t* niter_out, int32_t* status_out) {
    const std::string what(w.what);
    if (!s->streamed) return fail(ELLHIP_E_INVALID, (what + ": the _streamed entry points take streamed batch handles only").c_str());
    if (s->variant != ELLHIP_SPACE_ELL) return fail(ELLHIP_E_INVALID, (what + ": EllStable batch handles are not supported").c_str());
    if (s->B != st.B || s->n != st.n)
        return fail(ELLHIP_E_INVALID, (what + ": spaces and oracle differ in B or n" + w.n_is).c_str());
    if (s->device != st.device) return fail(ELLHIP_E_INVALID, (what + ": spaces and oracle live on different devices").c_str());
    const size_t lds = batch_streamed_loop_lds_doubles<Oracle>(A, s->n) * sizeof(double);
    if (lds > BATCH_LOOP_LDS_MAX)
        return fail(ELLHIP_E_INVALID, (what + ": this " + w.shape + " needs more LDS than a workgroup has").c_str());
    BatchStreamedParams P;
    P.B = s->B;
    P.n = s->n;
    P.np = batch_streamed_np(s->n);
    P.K = 0;
    P.no_defer_trick = s->no_defer_trick;
    const EllCalcDev calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    const BatchLoopState S = batch_loop_view(st);
    return batch_loop_drive(s, st, feas, gamma_inout, max_iters, tol, x_out, has_out, niter_out, status_out,
                            [&](const BatchLoopRun& R) {
        if (const int rc = batch_streamed_allow_lds<Oracle>(reinterpret_cast<const void*>(&k_batch_streamed_loop<Oracle>),
                                                            s->device, 0, lds))
            return rc;
        hipLaunchKernelGGL(k_batch_streamed_loop<Oracle>, dim3((unsigned)s->B), dim3(s->T), lds, s->stream, P, R, s->d_Q, s->d_xc,
                           s->d_kappa, s->d_tsq, s->d_sym, S, A, calc);
        return 0;
    });
}

int batch_lowpass_run_streamed(ellhip_batch* s, ellhip_batch_lowpass* o, int feas, double* gamma_inout, int64_t max_iters,
                               double tol, double* x_out, int32_t* has_out, int64_t* niter_out, int32_t* status_out) {
    if (!s || !o || !has_out || !niter_out || !status_out || (!feas && !gamma_inout))
        return fail(ELLHIP_E_INVALID, "NULL argument");
    return batch_streamed_loop_run<BatchLpOracle>(s, o->loop, batch_lowpass_args(o), {"batched lowpass streamed loop", "n", ""},
                                                  feas, gamma_inout, max_iters, tol, x_out, has_out, niter_out, status_out);
}

}  // namespace

extern "C" {

int ellhip_batch_lowpass_create_streamed(ellhip_batch_lowpass** out, int64_t B, int64_t n, const double* wpass,
                                         const double* wstop, const double* lp_sq, const double* up_sq, const double* sp_sq,
                                         const double* spectrum, int device) {
    return batch_lowpass_create(out, B, n, wpass, wstop, lp_sq, up_sq, sp_sq, spectrum, device, BATCH_STREAMED_NMAX);
}

int ellhip_batch_lowpass_optim_streamed(ellhip_batch* spaces, ellhip_batch_lowpass* o, double* gamma_inout, int64_t max_iters,
                                        double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                        int32_t* status_out) {
    return batch_lowpass_run_streamed(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out,
                                      status_out);
}

int ellhip_batch_lowpass_feas_streamed(ellhip_batch* spaces, ellhip_batch_lowpass* o, int64_t max_iters, double tol,
                                       double* x_out, int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lowpass_run_streamed(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out);
}

}  // extern "C"
