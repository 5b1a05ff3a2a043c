// batch_svm_streamed_capi.inc.hpp -- C ABI of the batched device-resident SVM cutting-plane loop on streamed batch handles,
// Ell and EllStable (include/ellhip_batch_svm_streamed.h).  Included at the end of ellhip_capi.hip,
// after batch_svm_capi.inc.hpp (the oracle handle, batch_svm_create and batch_svm_run, which reaches both kernels through
// batch_loop_run of batch_loop_capi.inc.hpp).
//
// Nothing here but two engines of that driver: k_batch_streamed_loop<BatchSvmOracle> and k_batch_streamed_loop_stable<BatchSvmOracle>
// take the policy k_batch_loop takes (batch_svm_kernels.hpp), whose scan is mapped onto "the n threads of an instance" with
// a stride of n and so is tied neither to an instance-per-workgroup count nor to n <= 128.  The block is n rounded up to 64
// threads; threads i >= n are inactive in the oracle (live = false) and take part in each of its barriers.  Bounds: every
// loop is bounded by iters, ceil(m / n), nfeat and n; no thread waits on another workgroup or on a memory word; the only
// global atomic is the stopped count (the two atomic minima of the argmin merge are on LDS words); the oracle is never
// called for a round the reference would not run, because min_idx and min_val are state the caller reads.
//
// Reference: src/oracles/svm_oracle.rs:4-58 (oracle), src/cutting_plane.rs:286-313 (loop).
#include "../../include/ellhip_batch_svm_streamed.h"

extern "C" {

int ellhip_batch_svm_create_streamed(ellhip_batch_svm** out, int64_t B, int64_t m, int64_t nfeat, const double* data,
                                     int32_t shared_data, const int32_t* labels, int device) {
    return batch_svm_create(out, B, m, nfeat, data, shared_data, labels, device, BATCH_STREAMED_NMAX - 1);
}

int ellhip_batch_svm_optim_streamed(ellhip_batch* spaces, ellhip_batch_svm* o, double* gamma_inout, int64_t max_iters,
                                    double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                    int32_t* status_out) {
    return batch_svm_run(spaces, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                         BATCH_ENGINE_STREAMED);
}

int ellhip_batch_svm_optim_streamed_stable(ellhip_batch* spaces, ellhip_batch_svm* o, double* gamma_inout, int64_t max_iters,
                                           double tol, double* x_best_out, int32_t* has_best_out, int64_t* niter_out,
                                           int32_t* status_out) {
    return batch_svm_run(spaces, o, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                         BATCH_ENGINE_STREAMED_STABLE);
}

}  // extern "C"
