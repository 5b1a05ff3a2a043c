// ellhip_capi.hip -- implementation of the C ABI declared in include/ellhip.h.
//
// The one translation unit of libellhip.so: the #include list, the extern "C" entry points of one search space, and the
// other engines.  The host-side runtime those entry points call -- the handle that owns the device buffers, the launchers
// of ell_kernels.hpp / ellstable_kernels.hpp, the schedulers -- is in the ell_*_capi.inc.hpp pieces included below.  No
// torch types, no CPU compute path: without a HIP device every entry point that needs one fails (ELLHIP_E_NODEVICE).
//
// Every update is built from three primitives (see include/ellhip.h, "pipelined update"):
//   prime   GEMV pass            gt[slot] = Q * g
//   cut     scalar stage         omega, tsq, EllCalc, xc, kappa   (EllStable: the whole update)
//   commit  rank-1 pass, optionally fused with the GEMV pass of the next gradient
// ellhip_update = prime + cut + commit(NULL); the two-phase multi-GPU form splits it after prime.
#include "../../include/ellhip.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ell_kernels.hpp"
#include "ellstable_kernels.hpp"
#include "resident_kernels.hpp"
#include "group_kernels.hpp"
#include "device_allocs.hpp"

using namespace ellhip;

// the engine of one search space, piece by piece ("where the engine's host code lives"); each header says what it needs
#include "launch_dispatch.hpp"
#include "ell_handle_capi.inc.hpp"
#include "ell_side_capi.inc.hpp"
#include "ell_passes_capi.inc.hpp"
#include "ellstable_capi.inc.hpp"
#include "ell_primitives_capi.inc.hpp"
#include "ell_queue_capi.inc.hpp"
#include "ell_group_capi.inc.hpp"
#include "ell_resident_capi.inc.hpp"

// ================================================================================= C ABI ======

extern "C" {

int ellhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* ellhip_last_error(void) { return g_last_error.c_str(); }

const char* ellhip_version(void) { return "ellhip 0.4.0 gfx950"; }

int ellhip_create(ellhip_space** out, int variant, int64_t n, double kappa, const double* mq, const double* diag,
                  const double* xc, int device) {
    return create_impl(out, variant, n, 0, n, false, kappa, mq, diag, xc, device);
}

int ellhip_create_shard(ellhip_space** out, int64_t n, int64_t row0, int64_t nrows, double kappa,
                        const double* mq_rows, const double* diag, const double* xc, int device) {
    return create_impl(out, ELLHIP_SPACE_ELL, n, row0, nrows, true, kappa, mq_rows, diag, xc, device);
}

void ellhip_destroy(ellhip_space* s) {
    if (!s) return;
    DeviceGuard guard(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->aux_stream) (void)hipStreamSynchronize(s->aux_stream);  // nothing may be in flight when the buffers go
    if (s->symv_stream) (void)hipStreamSynchronize(s->symv_stream);
    s->mem.release_all();  // (while the guard is alive, before the streams go)
    for (auto& pe : s->prof_events) {
        (void)hipEventDestroy(pe.a);
        (void)hipEventDestroy(pe.b);
    }
    if (s->ev_symv) (void)hipEventDestroy(s->ev_symv);
    if (s->ev_side_go) (void)hipEventDestroy(s->ev_side_go);
    if (s->symv_stream) (void)hipStreamDestroy(s->symv_stream);
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    if (s->aux_stream) (void)hipStreamDestroy(s->aux_stream);
    if (s->own_stream) (void)hipStreamDestroy(s->own_stream);
    delete s;
}

int ellhip_clone(const ellhip_space* src_c, ellhip_space** out) {
    if (!src_c || !out) return fail(ELLHIP_E_INVALID, "NULL argument");
    *out = nullptr;
    ellhip_space* src = const_cast<ellhip_space*>(src_c);  // committing a pending shrink is not observable
    DeviceGuard guard(src->device);
    int rc = make_q_current(src);
    if (rc) return rc;
    ellhip_space* s = new (std::nothrow) ellhip_space();
    if (!s) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    static_cast<SpaceInherited&>(*s) = *src;  // what a clone inherits, as one record ...
    static_cast<SpaceOptions&>(*s) = *src;    // ... and every option; not rs_fault_at (the test hook stays with its handle)
    s->kappa = src->kappa;
    s->tsq = src->tsq;
    rc = alloc_common(s);
    if (rc) {
        ellhip_destroy(s);
        return rc;
    }
    // order the copies after everything the source has in flight
    hipError_t e = hipStreamSynchronize(src->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(s->d_Q, src->d_Q, (size_t)s->nrows * (size_t)s->ld * sizeof(double),
                           hipMemcpyDeviceToDevice, s->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(s->d_xc, src->d_xc, (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, s->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_st, src->d_st, sizeof(DevState), hipMemcpyDeviceToDevice, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        ellhip_destroy(s);
        return fail(ELLHIP_E_HIP, "clone copy", e);
    }
    // The device state is the truth (the source's host cache lags behind asynchronous queue cuts); the clone has no
    // queue, so it does not inherit a halted one.
    rc = read_back(s);
    if (!rc) {
        s->h_result->halted = 0;
        s->h_result->halted_in = 0;
        s->h_result->stop = STOP_NONE;
        s->h_result->tol = -1.0;
        s->h_result->niter = 0;
        e = hipMemcpyAsync(s->d_st, s->h_result, sizeof(DevState), hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) rc = fail(ELLHIP_E_HIP, "clone state", e);
    }
    if (rc) {
        ellhip_destroy(s);
        return rc;
    }
    if (src->defer > 1) {
        rc = ellhip_set_defer_depth(s, src->defer);
        if (rc) {
            ellhip_destroy(s);
            return rc;
        }
    }
    *out = s;
    return 0;
}

// ---- pipelined primitives ---------------------------------------------------------------------

int ellhip_prime(ellhip_space* s, const double* grad) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(s->device);
    int rc = ensure_committed(s);
    if (rc) return rc;
    // re-priming over a gradient that may still be uploading: let the stream drain before the pinned
    // staging buffer of this slot is overwritten
    if (s->primed) HIPCHK(hipStreamSynchronize(s->stream));
    rc = stage_grad(s, grad, s->cur);
    if (rc) return rc;
    rc = do_prime(s, s->d_stage[s->cur], s->cur);
    if (rc) return rc;
    s->primed = true;
    s->g_cur = s->d_stage[s->cur];
    s->primed_qindex = -1;
    return 0;
}

int ellhip_cut(ellhip_space* s, int kind, double beta0, int has_beta1, double beta1) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (!s->primed) return fail(ELLHIP_E_STATE, "ellhip_cut without a primed gradient");
    if (s->shrink_pending) return fail(ELLHIP_E_STATE, "ellhip_cut: previous cut not committed");
    DeviceGuard guard(s->device);
    CutParams cp;
    int rc = make_params(kind, beta0, has_beta1, beta1, cp);
    if (rc) return rc;
    s->live_arm = true;
    rc = do_cut(s, s->g_cur, nullptr, cp, 0, nullptr, nullptr);
    s->live_arm = false;
    if (rc) s->live_done = false;
    if (!rc) rc = live_publish(s);
    if (!rc) rc = live_wait(s);
    if (rc) return rc;
    const int status = s->h_result->status;
    s->npend = s->h_result->npend;  // deferred mode: a failed cut records nothing
    s->shrink_pending = (status == ELLHIP_SUCCESS) && s->variant == ELLHIP_SPACE_ELL && !deferring(s);
    s->primed = false;  // the gradient has been consumed; gt[cur] stays valid for the pending shrink
    return status;
}

int ellhip_commit(ellhip_space* s, const double* next_grad) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (s->in_two_phase) return fail(ELLHIP_E_STATE, "update_begin without update_end");
    DeviceGuard guard(s->device);
    const int nslot = s->cur ^ 1;
    if (next_grad) {
        int rc = stage_grad(s, next_grad, nslot);
        if (rc) return rc;
    }
    const bool shrink = s->shrink_pending;
    int rc = do_commit(s, shrink, next_grad ? s->d_stage[nslot] : nullptr);
    if (rc) return rc;
    if (shrink) s->needs_mirror = false;  // the mirror ran ahead of this successful shrink
    s->shrink_pending = false;
    if (next_grad) {
        s->cur = nslot;
        s->primed = true;
        s->g_cur = s->d_stage[nslot];
        s->primed_qindex = -1;
    } else {
        drop_prime(s);
    }
    return 0;
}

// ---- the SearchSpace update and its two-phase form ------------------------------------------------

int ellhip_update_begin(ellhip_space* s, int kind, const double* grad, double beta0, int has_beta1, double beta1) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (s->in_two_phase) return fail(ELLHIP_E_STATE, "update_begin called twice");
    if (!grad) return fail(ELLHIP_E_INVALID, "grad is NULL");
    CutParams cp;
    int rc = make_params(kind, beta0, has_beta1, beta1, cp);
    if (rc) return rc;
    rc = ellhip_prime(s, grad);
    if (rc) return rc;
    s->two_phase_cp = cp;
    s->in_two_phase = true;
    return 0;
}

int ellhip_update_end(ellhip_space* s) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (!s->in_two_phase) return fail(ELLHIP_E_STATE, "update_end without update_begin");
    DeviceGuard guard(s->device);
    s->in_two_phase = false;
    s->live_arm = true;
    int rc = do_cut(s, s->g_cur, nullptr, s->two_phase_cp, 0, nullptr, nullptr);
    s->live_arm = false;
    if (rc) {
        s->live_done = false;
        return rc;
    }
    // status, tsq, kappa and the new centre are final after the scalar stage: they go to the host from there
    rc = live_publish(s);
    if (rc) return rc;
    // the rank-1 pass (or, on the recorded schedule, the apply pass when the slots are full) is skipped on the device when
    // the cut failed, so it is issued before the status is known -- and nobody waits for it: the caller's next statements
    // (status test, tsq, xc(), its oracle) run beside it, the next update on this handle is ordered behind it by the stream
    rc = do_commit(s, true, nullptr);
    if (rc) return rc;
    drop_prime(s);
    rc = live_wait(s);
    if (rc) return rc;
    const int status = s->h_result->status;
    if (s->variant == ELLHIP_SPACE_ELL && s->npend > 0 && status != ELLHIP_SUCCESS && s->h_result->npend < s->npend)
        s->npend = s->h_result->npend;  // deferred mode: the failed cut recorded nothing
    if (status == ELLHIP_SUCCESS) s->needs_mirror = false;
    return status;
}

int ellhip_update(ellhip_space* s, int kind, const double* grad, double beta0, int has_beta1, double beta1) {
    int rc = ellhip_update_begin(s, kind, grad, beta0, has_beta1, beta1);
    if (!rc) rc = ellhip_update_end(s);
    return rc;
}

namespace {
// kappa / tsq are cached on the host by every synchronous call; after asynchronous queue cuts they are fetched
void refresh_scalars(const ellhip_space* s_c) {
    if (!s_c->scalars_stale) return;
    ellhip_space* s = const_cast<ellhip_space*>(s_c);
    DeviceGuard guard(s->device);
    (void)read_back(s);
}
}  // namespace

double ellhip_tsq(const ellhip_space* s) {
    if (!s) return 0.0;
    refresh_scalars(s);
    return s->tsq;
}
double ellhip_kappa(const ellhip_space* s) {
    if (!s) return 0.0;
    refresh_scalars(s);
    return s->kappa;
}
int64_t ellhip_ndim(const ellhip_space* s) { return s ? s->n : 0; }

int ellhip_get_xc(const ellhip_space* s, double* xc_out) {
    if (!s || !xc_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    if (s->xc_host_valid) {  // published by the last direct update (k_publish): no device call at all
        memcpy(xc_out, s->h_xc, (size_t)s->n * sizeof(double));
        return 0;
    }
    DeviceGuard guard(s->device);
    HIPCHK(hipMemcpyAsync(xc_out, s->d_xc, (size_t)s->n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

int ellhip_set_xc(ellhip_space* s, const double* xc) {
    if (!s || !xc) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(s->device);
    // staged through the slot that is NOT holding a primed gradient
    s->xc_host_valid = false;
    const int slot = s->cur ^ 1;
    HIPCHK(hipStreamSynchronize(s->stream));
    memcpy(s->h_stage[slot], xc, (size_t)s->n * sizeof(double));
    HIPCHK(hipMemcpyAsync(s->d_xc, s->h_stage[slot], (size_t)s->n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

int ellhip_get_mq(const ellhip_space* s_c, double* mq_out) {
    if (!s_c || !mq_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    ellhip_space* s = const_cast<ellhip_space*>(s_c);
    DeviceGuard guard(s->device);
    int rc = make_q_current(s);
    if (rc) return rc;
    HIPCHK(hipMemcpy2DAsync(mq_out, (size_t)s->n * sizeof(double), s->d_Q, (size_t)s->ld * sizeof(double),
                            (size_t)s->n * sizeof(double), (size_t)s->nrows, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

int ellhip_set_no_defer_trick(ellhip_space* s, int flag) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (s->variant != ELLHIP_SPACE_ELL) return fail(ELLHIP_E_INVALID, "no_defer_trick exists on Ell only");
    if (s->shard_symmetric && flag) return fail(ELLHIP_E_STATE, "symmetric row shard: no_defer_trick is not available");
    DeviceGuard guard(s->device);
    int rc = make_q_current(s);  // recorded updates belong to the old mode
    if (rc) return rc;
    s->no_defer_trick = flag ? 1 : 0;
    return 0;
}

int ellhip_set_defer_depth(ellhip_space* s, int depth) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (s->variant != ELLHIP_SPACE_ELL) return fail(ELLHIP_E_INVALID, "deferred shrink exists on Ell only");
    if (depth != 1 && depth != 8 && depth != 16 && depth != 24) return fail(ELLHIP_E_INVALID, "defer depth must be 1, 8, 16 or 24");
    if (s->shard_symmetric && depth == 1 && s->upper_stale)
        return fail(ELLHIP_E_STATE, "symmetric row shard: the rows are current up to their diagonal only");
    DeviceGuard guard(s->device);
    int rc = make_q_current(s);
    if (rc) return rc;
    if (depth > 1) {
        rc = symv_alloc(s);
        if (rc) return rc;
    }
    if (depth >= 16) {
        // 16 / 24 pending updates only fit the lower-triangle schedule (k_symv + k_apply_lower)
        const bool lower_schedule = s->symv && s->apply_lower && (s->n % 2) == 0 && s->d_rowpart &&
                                    (s->sharded ? s->shard_symmetric : s->n >= s->symv_min_n);
        if (!lower_schedule)
            return fail(ELLHIP_E_INVALID, "defer depth 16 / 24 needs the lower-triangle schedule: an unsharded handle with n "
                                          "even and >= ELLHIP_OPT_SYMV_MIN_N (5120 by default), or a symmetric row shard");
    }
    s->defer = depth;
    return 0;
}

int ellhip_defer_depth(const ellhip_space* s) { return s ? s->defer : 0; }

int ellhip_flush(ellhip_space* s) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (s->variant != ELLHIP_SPACE_ELL) return 0;
    DeviceGuard guard(s->device);
    const bool uncut = prime_is_uncut(s);
    int rc = ensure_committed(s);
    if (rc) return rc;
    if (s->npend > 0) {
        rc = flush_pending(s, nullptr, nullptr);
        if (rc) return rc;
        if (uncut) return refresh_prime(s);  // the primed gradient's Q_base*g belongs to the old base
    }
    return 0;
}

int64_t ellhip_queue_primed(const ellhip_space* s) { return (s && s->primed) ? (int64_t)s->primed_qindex : -1; }

int ellhip_set_shard_symmetric(ellhip_space* s, int flag) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (!s->sharded || s->variant != ELLHIP_SPACE_ELL) return fail(ELLHIP_E_INVALID, "symmetric mode is for row shards of Ell");
    if ((s->n % 2) != 0 || (s->row0 % SYMV_H) != 0 || ((s->row0 + s->nrows) % SYMV_H != 0 && s->row0 + s->nrows != s->n))
        return fail(ELLHIP_E_INVALID, "symmetric row shard: n must be even and the shard boundaries multiples of 64");
    if (s->in_two_phase || s->primed || s->shrink_pending || s->npend > 0 || s->upper_stale)
        return fail(ELLHIP_E_STATE, "symmetric row shard: set the mode before the first update");
    DeviceGuard guard(s->device);
    s->shard_symmetric = flag != 0;
    if (s->shard_symmetric && s->defer > 1) {
        int rc = symv_alloc(s);
        if (rc) return rc;
    }
    return 0;
}

int ellhip_set_use_parallel_cut(ellhip_space* s, int flag) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    s->use_parallel_cut = flag ? 1 : 0;
    return 0;
}

int ellhip_calc(int64_t n, int use_parallel_cut, int kind, double beta0, int has_beta1, double beta1, double tsq,
                double* out3, int device) {
    if (!out3 || n < 1 || kind < 0 || kind > 2) return fail(ELLHIP_E_INVALID, "bad argument");
    if (ellhip_device_count() <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    DeviceGuard guard(device);
    Allocs tmp;
    double* d_out = nullptr;  // (freed on every return path)
    HIPCHK(tmp.device(d_out, 4 * sizeof(double)));
    CutParams cp;
    cp.kind = kind;
    cp.has_b1 = has_beta1 ? 1 : 0;
    cp.b0 = beta0;
    cp.b1 = has_beta1 ? beta1 : 0.0;
    hipLaunchKernelGGL(k_calc_one, dim3(1), dim3(1), 0, 0, EllCalcDev::make(n, use_parallel_cut), cp, tsq, d_out);
    double h[4];
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(h, d_out, sizeof h, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ELLHIP_E_HIP, "ellhip_calc", e);
    out3[0] = h[1];
    out3[1] = h[2];
    out3[2] = h[3];
    return (int)h[0];
}

double* ellhip_gt_dev(ellhip_space* s) { return s ? s->d_gt[s->cur] : nullptr; }

int ellhip_set_gt_dev(ellhip_space* s, double* gt_dev_a, double* gt_dev_b) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (s->in_two_phase || s->primed || s->shrink_pending) return fail(ELLHIP_E_STATE, "update in flight");
    s->d_gt[0] = gt_dev_a ? gt_dev_a : s->d_gt_own[0];
    s->d_gt[1] = gt_dev_b ? gt_dev_b : s->d_gt_own[1];
    return 0;
}

// ---- queue ------------------------------------------------------------------------------------

int ellhip_queue_upload(ellhip_space* s, int64_t k, const int32_t* kinds, const double* grads, const double* beta0,
                        const int32_t* has_beta1, const double* beta1) {
    if (!s || k < 1 || !kinds || !grads || !beta0) return fail(ELLHIP_E_INVALID, "bad argument");
    DeviceGuard guard(s->device);
    int rc = ensure_committed(s);
    if (rc) return rc;
    drop_prime(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    queue_free(s);
    const long long n = s->n;
    std::vector<CutParams> hp((size_t)k);
    for (int64_t i = 0; i < k; ++i) {
        if (kinds[i] < 0 || kinds[i] > 2) return fail(ELLHIP_E_INVALID, "bad cut kind in queue");
        hp[(size_t)i].kind = kinds[i];
        hp[(size_t)i].has_b1 = (has_beta1 && has_beta1[i]) ? 1 : 0;
        hp[(size_t)i].b0 = beta0[i];
        hp[(size_t)i].b1 = (has_beta1 && has_beta1[i] && beta1) ? beta1[i] : 0.0;
    }
    // the four buffers and their contents, or no queue at all (qk == 0, every pointer null)
    hipError_t e = s->mem.device(s->d_qparams, (size_t)k * sizeof(CutParams));
    if (e == hipSuccess) e = s->mem.device(s->d_qgrads, (size_t)k * (size_t)n * sizeof(double));
    if (e == hipSuccess) e = s->mem.device(s->d_qstatus, (size_t)k * sizeof(int));
    if (e == hipSuccess) e = s->mem.device(s->d_qtsq, (size_t)k * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(s->d_qparams, hp.data(), (size_t)k * sizeof(CutParams), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_qgrads, grads, (size_t)k * (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = fill_now(s->d_qstatus, 0xff, (size_t)k * sizeof(int), s->stream);  // -1 = not run yet
    if (e == hipSuccess) e = fill_now(s->d_qtsq, 0, (size_t)k * sizeof(double), s->stream);
    if (e != hipSuccess) {
        queue_free(s);
        return fail(ELLHIP_E_HIP, "ellhip_queue_upload", e);
    }
    s->qk = k;
    return 0;
}

int ellhip_queue_prime(ellhip_space* s, int64_t index) {
    int rc = queue_index_ok(s, index);
    if (rc) return rc;
    DeviceGuard guard(s->device);
    return queue_prime_impl(s, index);
}

int ellhip_queue_cut(ellhip_space* s, int64_t index) {
    int rc = queue_index_ok(s, index);
    if (rc) return rc;
    DeviceGuard guard(s->device);
    return queue_cut_impl(s, index);
}

int ellhip_queue_commit(ellhip_space* s, int64_t index, int64_t next_index) {
    int rc = queue_index_ok(s, index);
    if (rc) return rc;
    if (next_index >= s->qk) return fail(ELLHIP_E_INVALID, "queue next_index out of range");
    DeviceGuard guard(s->device);
    return queue_commit_impl(s, index, next_index);
}

int ellhip_queue_begin(ellhip_space* s, int64_t index) { return ellhip_queue_prime(s, index); }

int ellhip_queue_end(ellhip_space* s, int64_t index) {
    int rc = ellhip_queue_cut(s, index);
    if (rc) return rc;
    return ellhip_queue_commit(s, index, -1);
}

int ellhip_queue_run(ellhip_space* s, int64_t first, int64_t count) {
    if (!s || first < 0 || count < 0 || first + count > s->qk) return fail(ELLHIP_E_INVALID, "queue range");
    DeviceGuard guard(s->device);
    if (resident_ok(s, count)) {
        const int rrc = resident_run(s, first, count);
        if (rrc != RS_FALLBACK) return rrc;
    }
    for (int64_t i = first; i < first + count; ++i) {
        int rc = queue_prime_impl(s, i);
        if (!rc) rc = queue_cut_impl(s, i);
        if (!rc) rc = queue_commit_impl(s, i, -1);
        if (rc) return rc;
    }
    return 0;
}

int ellhip_queue_run_fused(ellhip_space* s, int64_t first, int64_t count) {
    if (!s || first < 0 || count < 0 || first + count > s->qk) return fail(ELLHIP_E_INVALID, "queue range");
    DeviceGuard guard(s->device);
    if (resident_ok(s, count)) {
        const int rrc = resident_run(s, first, count);
        if (rrc != RS_FALLBACK) return rrc;
    }
    if (multi_ok(s)) {
        const int mrc = queue_run_multi(s, first, count);
        if (mrc != MULTI_NO_MEMORY) return mrc;
    }
    if (overlap_ok(s)) return queue_run_overlapped(s, first, count);
    for (int64_t i = first; i < first + count; ++i) {
        int rc = queue_prime_impl(s, i);  // (pipelined form: only the first cut of a run pays a separate GEMV pass)
        if (!rc) rc = queue_cut_impl(s, i);
        if (!rc) rc = queue_commit_impl(s, i, (i + 1 < s->qk) ? i + 1 : -1);
        if (rc) return rc;
    }
    return 0;
}

int ellhip_queue_results(ellhip_space* s, int32_t* status_out, double* tsq_out) {
    if (!s || s->qk < 1) return fail(ELLHIP_E_INVALID, "no queue");
    DeviceGuard guard(s->device);
    int rc = read_back(s);
    if (rc) return rc;
    if (s->variant == ELLHIP_SPACE_ELL && s->h_result->halted) s->npend = s->h_result->npend;
    std::vector<int32_t> st((size_t)s->qk);
    HIPCHK(hipMemcpy(st.data(), s->d_qstatus, (size_t)s->qk * sizeof(int), hipMemcpyDeviceToHost));
    if (status_out) memcpy(status_out, st.data(), (size_t)s->qk * sizeof(int));
    if (tsq_out) HIPCHK(hipMemcpy(tsq_out, s->d_qtsq, (size_t)s->qk * sizeof(double), hipMemcpyDeviceToHost));
    if (s->needs_mirror) {
        for (int64_t i = 0; i < s->qk; ++i)
            if (st[(size_t)i] == ELLHIP_SUCCESS) {
                s->needs_mirror = false;
                break;
            }
    }
    // a halted queue stays halted until its results have been read; then direct updates work again
    if (s->h_result->halted && s->variant == ELLHIP_SPACE_ELL_STABLE) {
        // (mirrored layout: a k_st_mirror_enter issued while the queue was halted did nothing; host and device agree again)
        rc = stable_mirror_leave(s);
        if (rc) return rc;
    }
    if (s->h_result->halted) {
        s->h_result->halted = 0;
        s->h_result->stop = STOP_NONE;
        HIPCHK(hipMemcpyAsync(s->d_st, s->h_result, sizeof(DevState), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        drop_prime(s);  // whatever was primed beyond the failing cut never ran
        s->shrink_pending = false;
    }
    return 0;
}

// ---- streams / timing -------------------------------------------------------------------------

int ellhip_set_stream(ellhip_space* s, void* hip_stream) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : s->own_stream;
    return 0;
}

int ellhip_synchronize(ellhip_space* s) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

int ellhip_profile_enable(ellhip_space* s, int flag) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    s->profile = flag != 0;
    return 0;
}

int ellhip_profile_read(ellhip_space* s, double* ms_out, int64_t* count_out) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(s->device);
    int rc = prof_flush(s);
    if (rc) return rc;
    for (int i = 0; i < ELLHIP_NKERNEL_CLASSES; ++i) {
        if (ms_out) ms_out[i] = s->prof_ms[i];
        if (count_out) count_out[i] = s->prof_cnt[i];
        s->prof_ms[i] = 0.0;
        s->prof_cnt[i] = 0;
    }
    return 0;
}

}  // extern "C"

#include "ell_options_capi.inc.hpp"

#include "lowpass_capi.inc.hpp"
#include "batch_capi.inc.hpp"
#include "batch_streamed_capi.inc.hpp"
#include "batch_streamed_stable_capi.inc.hpp"
#include "lmi_capi.inc.hpp"
#include "sharded_capi.inc.hpp"
#include "svm_capi.inc.hpp"
#include "batch_loop_capi.inc.hpp"
#include "batch_lmi_capi.inc.hpp"
#include "batch_lowpass_capi.inc.hpp"
#include "batch_svm_capi.inc.hpp"
#include "lmi_loop_capi.inc.hpp"
#include "batch_stable_loops_capi.inc.hpp"
#include "batch_lowpass_streamed_capi.inc.hpp"
#include "batch_lowpass_streamed_stable_capi.inc.hpp"
#include "batch_svm_streamed_capi.inc.hpp"
#include "batch_lmi_streamed_capi.inc.hpp"
#include "batch_maxcut_capi.inc.hpp"
#include "batch_profit_capi.inc.hpp"
#include "batch_linfeas_capi.inc.hpp"
#include "batch_linfeas_streamed_capi.inc.hpp"
