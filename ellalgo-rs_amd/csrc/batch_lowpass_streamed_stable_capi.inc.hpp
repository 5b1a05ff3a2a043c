// batch_lowpass_streamed_stable_capi.inc.hpp -- C ABI of the batched device-resident low-pass design loop on a streamed
// EllStable batch handle (include/ellhip_batch_lowpass_streamed_stable.h).  Included at the end of ellhip_capi.hip, after
// batch_lowpass_capi.inc.hpp (the oracle handle and batch_lowpass_run, which reaches
// k_batch_streamed_loop_stable<BatchLpOracle> of batch_streamed_stable_loop_kernels.hpp through batch_loop_run of
// batch_loop_capi.inc.hpp).  The oracle handle is ellhip_batch_lowpass_create_streamed's.
#include "../../include/ellhip_batch_lowpass_streamed_stable.h"

extern "C" {

int ellhip_batch_lowpass_optim_streamed_stable(ellhip_batch* spaces, ellhip_batch_lowpass* o, double* gamma_inout,
                                               int64_t max_iters, double tol, double* x_best_out, int32_t* has_best_out,
                                               int64_t* niter_out, int32_t* status_out) {
    return batch_lowpass_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                             BATCH_ENGINE_STREAMED_STABLE);
}

int ellhip_batch_lowpass_feas_streamed_stable(ellhip_batch* spaces, ellhip_batch_lowpass* o, int64_t max_iters, double tol,
                                              double* x_out, int32_t* feasible_out, int64_t* niter_out,
                                              int32_t* status_out) {
    return batch_lowpass_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                             BATCH_ENGINE_STREAMED_STABLE);
}

}  // extern "C"
