// batch_lmi_streamed_capi.inc.hpp -- C ABI of the batched device-resident LMI cutting-plane loops on streamed batch handles,
// Ell and EllStable (include/ellhip_batch_lmi_streamed.h).  Included at the end of ellhip_capi.hip,
// after batch_lmi_capi.inc.hpp (the oracle handle, batch_lmi_create and batch_lmi_run, which reaches both kernels through
// batch_loop_run of batch_loop_capi.inc.hpp).
//
// Nothing here but two engines of that driver: k_batch_streamed_loop<BatchLmiOracle> and k_batch_streamed_loop_stable<BatchLmiOracle>
// take the policy k_batch_loop takes (batch_lmi_kernels.hpp), whose F(x), factor rows and quadratic forms are mapped onto "the
// n threads of an instance" with a stride of n and so are tied neither to an instance-per-workgroup count nor to n <= 128.
// The block is n rounded up to 64 threads; threads i >= n are inactive in the oracle (live = false) and take part in each of
// its barriers and votes.  LDS is the engine's own plus batch_lmi_lds_doubles(n, M): 89.2 KiB (Ell) and 81.7 KiB (EllStable)
// at n = 1024, M = 64, past the 64 KiB a kernel may use unasked, so the driver opts in (batch_loop_allow_lds).
//
// Bounds: every loop is bounded by iters, J + 1, M and n; every thread of the padded block reaches every barrier and vote;
// no thread waits on another workgroup or on a memory word; the only global atomic is the stopped count; the oracle is never
// called for a round the reference would not run, because idx and gamma are state the caller reads (the streamed loop's early
// call for round k + 1 is made only when that round runs in this launch).
//
// Reference: tests/lmi_tests.rs:142-171 (oracle), src/oracles/lmi_oracle.rs, lmi0_oracle.rs, ldlt_mgr.rs,
// src/cutting_plane.rs:205-227, 286-313 (loops).
#include "../../include/ellhip_batch_lmi_streamed.h"

extern "C" {

int ellhip_batch_lmi_create_streamed(ellhip_batch_lmi** out, int64_t B, int64_t n, int64_t J, const int64_t* m,
                                     const double* mat_f, int32_t shared_f, const double* mat_b, const double* c, int device) {
#ifdef ELLHIP_BATCH_LMI_FX_PENCIL  // measurement only: F(x) from the k-fastest pencil at every n
    return batch_lmi_create(out, B, n, J, m, mat_f, shared_f, mat_b, c, device, BATCH_STREAMED_NMAX, false);
#else
    return batch_lmi_create(out, B, n, J, m, mat_f, shared_f, mat_b, c, device, BATCH_STREAMED_NMAX, true);
#endif
}

int ellhip_batch_lmi_optim_streamed(ellhip_batch* spaces, ellhip_batch_lmi* o, double* gamma_inout, int64_t max_iters,
                                    double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                    int32_t* status_out) {
    return batch_lmi_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                         BATCH_ENGINE_STREAMED);
}

int ellhip_batch_lmi_feas_streamed(ellhip_batch* spaces, ellhip_batch_lmi* o, int64_t max_iters, double tol, double* x_out,
                                   int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lmi_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                         BATCH_ENGINE_STREAMED);
}

int ellhip_batch_lmi_optim_streamed_stable(ellhip_batch* spaces, ellhip_batch_lmi* o, double* gamma_inout, int64_t max_iters,
                                           double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                           int32_t* status_out) {
    return batch_lmi_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                         BATCH_ENGINE_STREAMED_STABLE);
}

int ellhip_batch_lmi_feas_streamed_stable(ellhip_batch* spaces, ellhip_batch_lmi* o, int64_t max_iters, double tol,
                                          double* x_out, int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lmi_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out,
                         BATCH_ENGINE_STREAMED_STABLE);
}

}  // extern "C"
