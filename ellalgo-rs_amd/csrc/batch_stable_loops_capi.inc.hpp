// batch_stable_loops_capi.inc.hpp -- C ABI of the batched device-resident cutting-plane loops on EllStable batch handles
// (include/ellhip_batch_stable_loops.h).  Included at the end of ellhip_capi.hip, after batch_lmi_capi.inc.hpp,
// batch_lowpass_capi.inc.hpp and batch_svm_capi.inc.hpp: it runs their launch helpers (batch_lmi_run, batch_lowpass_run,
// batch_svm_run) on BATCH_ENGINE_LDS_STABLE: the EllStable instantiation of k_batch_loop (batch_loop_kernels.hpp,
// batch_stable_apply.hpp), so the checks, the chunked relaunch and the copies out are the Ell entry points' own (batch_loop_run).
//
// Reference: src/ell_stable.rs:52-125 (update_core), :139-153 (update_bias_cut / update_central_cut),
// src/cutting_plane.rs:205-227, 286-313 (loops), tests/lmi_tests.rs:201-225 (the LMI problems on EllStable).
#include "../../include/ellhip_batch_stable_loops.h"

extern "C" {

int ellhip_batch_lmi_optim_stable(ellhip_batch* spaces, ellhip_batch_lmi* o, double* gamma_inout, int64_t max_iters,
                                  double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                  int32_t* status_out) {
    return batch_lmi_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                         BATCH_ENGINE_LDS_STABLE);
}

int ellhip_batch_lmi_feas_stable(ellhip_batch* spaces, ellhip_batch_lmi* o, int64_t max_iters, double tol, double* x_out,
                                 int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lmi_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                         BATCH_ENGINE_LDS_STABLE);
}

int ellhip_batch_lowpass_optim_stable(ellhip_batch* spaces, ellhip_batch_lowpass* o, double* gamma_inout, int64_t max_iters,
                                      double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                      int32_t* status_out) {
    return batch_lowpass_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                             BATCH_ENGINE_LDS_STABLE);
}

int ellhip_batch_lowpass_feas_stable(ellhip_batch* spaces, ellhip_batch_lowpass* o, int64_t max_iters, double tol,
                                     double* x_out, int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lowpass_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                             BATCH_ENGINE_LDS_STABLE);
}

int ellhip_batch_svm_optim_stable(ellhip_batch* spaces, ellhip_batch_svm* o, double* gamma_inout, int64_t max_iters,
                                  double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                  int32_t* status_out) {
    return batch_svm_run(spaces, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                         BATCH_ENGINE_LDS_STABLE);
}

}  // extern "C"
