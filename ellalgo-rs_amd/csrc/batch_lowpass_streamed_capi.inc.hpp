// batch_lowpass_streamed_capi.inc.hpp -- C ABI of the batched device-resident low-pass design loop on a streamed batch handle
// (include/ellhip_batch_lowpass_streamed.h).  Included at the end of ellhip_capi.hip, after batch_lowpass_capi.inc.hpp (the
// oracle handle, batch_lowpass_create and batch_lowpass_run, which reaches k_batch_streamed_loop<BatchLpOracle> of
// batch_streamed_loop_kernels.hpp through batch_loop_run of batch_loop_capi.inc.hpp).
#include "../../include/ellhip_batch_lowpass_streamed.h"

extern "C" {

int ellhip_batch_lowpass_create_streamed(ellhip_batch_lowpass** out, int64_t B, int64_t n, const double* wpass,
                                         const double* wstop, const double* lp_sq, const double* up_sq, const double* sp_sq,
                                         const double* spectrum, int device) {
    return batch_lowpass_create(out, B, n, wpass, wstop, lp_sq, up_sq, sp_sq, spectrum, device, BATCH_STREAMED_NMAX);
}

int ellhip_batch_lowpass_optim_streamed(ellhip_batch* spaces, ellhip_batch_lowpass* o, double* gamma_inout, int64_t max_iters,
                                        double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                        int32_t* status_out) {
    return batch_lowpass_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                             BATCH_ENGINE_STREAMED);
}

int ellhip_batch_lowpass_feas_streamed(ellhip_batch* spaces, ellhip_batch_lowpass* o, int64_t max_iters, double tol,
                                       double* x_out, int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lowpass_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                             BATCH_ENGINE_STREAMED);
}

}  // extern "C"
