// device_loop.inc.hpp -- the device-resident cutting-plane loop shared by the device-side oracles (lowpass_capi.inc.hpp,
// svm_capi.inc.hpp).  Included by them inside the one translation unit of ellhip_capi.hip: it issues the search-space
// primitives do_prime / do_cut / do_commit (ell_primitives_capi.inc.hpp) directly.
//
// Reference: src/cutting_plane.rs:205-227,286-313.  The host enqueues iterations in batches of DL_BATCH; every kernel of
// an iteration (the oracle's, GEMV, scalar stage, shrink) is a no-op once the loop has halted on the device, so the host
// looks at the state once per batch only.  The oracle for iteration k+1 runs between the scalar stage and the shrink of
// iteration k, which then carries the next GEMV.
//
// A Stage is the oracle's side of the loop:
//   hipStream_t stream()                                   the oracle's own stream (drained before the loop starts)
//   int begin(hipStream_t st)                              reset the oracle's loop outputs (has_best, gamma, errors)
//   int issue(hipStream_t st, ellhip_space* s, const int* halted)
//                                                          this iteration's oracle kernels at s->d_xc; they write the
//                                                          gradient grad() and the cut values cut(), and may halt the loop
//   const double* grad();  const CutParams* cut();
//   int finish(hipStream_t st, long long niter)
//                                                          read back best / gamma / error once the loop is over
#pragma once

namespace {

constexpr long long DL_BATCH = 64;

template <class Stage>
int drive_device_loop(ellhip_space* s, Stage& stage, long long n, int device, long long max_iters, double tol) {
    if (s->n != n) return fail(ELLHIP_E_INVALID, "oracle and search space dimensions differ");
    if (s->device != device) return fail(ELLHIP_E_INVALID, "oracle and search space live on different devices");
    if (s->sharded) return fail(ELLHIP_E_INVALID, "device-resident loops need an unsharded search space");
    if (max_iters < 0) return fail(ELLHIP_E_INVALID, "max_iters < 0");
    DeviceGuard guard(s->device);
    int rc = ensure_committed(s);
    if (rc) return rc;
    drop_prime(s);
    HIPCHK(hipStreamSynchronize(stage.stream()));
    hipStream_t st = s->stream;
    // loop state on the device: tolerance, iteration counter, stop reason
    rc = read_back(s);
    if (rc) return rc;
    s->h_result->tol = tol;
    s->h_result->niter = 0;
    s->h_result->stop = STOP_NONE;
    s->h_result->halted = 0;
    HIPCHK(hipMemcpyAsync(s->d_st, s->h_result, sizeof(DevState), hipMemcpyHostToDevice, st));
    rc = stage.begin(st);
    if (rc) return rc;

    int* d_halted = reinterpret_cast<int*>(reinterpret_cast<char*>(s->d_st) + offsetof(DevState, halted));
    std::vector<int> slot_of((size_t)DL_BATCH);
    long long done = 0;
    CutParams none{};
    bool stopped = false;
    while (done < max_iters && !stopped) {
        const long long nb = (max_iters - done < DL_BATCH) ? max_iters - done : DL_BATCH;
        for (long long i = 0; i < nb; ++i) {
            // oracle at the current centre; for every iteration but the first of a batch it runs between the
            // scalar stage of the previous cut and that cut's shrink, which then carries this cut's GEMV
            rc = stage.issue(st, s, d_halted);
            if (rc) return rc;
            if (s->shrink_pending || (deferring(s) && i > 0)) {
                rc = do_commit(s, s->shrink_pending, stage.grad());
                if (rc) return rc;
                s->shrink_pending = false;
                s->cur ^= 1;
            } else {
                rc = do_prime(s, stage.grad(), s->cur);
                if (rc) return rc;
            }
            slot_of[(size_t)i] = s->cur;
            rc = do_cut(s, stage.grad(), stage.cut(), none, 1, nullptr, nullptr);
            if (rc) return rc;
            s->shrink_pending = s->variant == ELLHIP_SPACE_ELL && !deferring(s);
        }
        // end of batch: apply the last shrink (it has no next gradient yet), then look at the loop state
        rc = do_commit(s, s->shrink_pending, nullptr);
        if (rc) return rc;
        s->shrink_pending = false;
        rc = read_back(s);
        if (rc) return rc;
        const DevState hs = *s->h_result;
        if (s->needs_mirror && (hs.niter > 0 || hs.stop == STOP_TOL)) s->needs_mirror = false;
        if (hs.halted) {
            stopped = true;
            const long long at = hs.niter - done;  // index of the stopping iteration inside this batch
            if (s->variant == ELLHIP_SPACE_ELL) s->npend = hs.npend;
            // clear the halt so that the space is usable again (and so that the shrink below runs)
            s->h_result->halted = 0;
            HIPCHK(hipMemcpyAsync(s->d_st, s->h_result, sizeof(DevState), hipMemcpyHostToDevice, st));
            if (hs.stop == STOP_TOL && s->variant == ELLHIP_SPACE_ELL && !deferring(s)) {
                // src/cutting_plane.rs:308 tests tsq AFTER the update: the update that hit the tolerance is
                // complete in the reference.  Its scalar stage set `halted`, which turned the shrink pass into a
                // no-op; gt of that cut is still in its slot and DevState.apply is still 1.
                if (at < 0 || at >= nb) return fail(ELLHIP_E_STATE, "device loop: inconsistent iteration count");
                s->cur = slot_of[(size_t)at];
                rc = do_commit(s, true, nullptr);
                if (rc) return rc;
            }
            if (hs.stop == STOP_FEASIBLE && s->variant == ELLHIP_SPACE_ELL && !deferring(s) && at > 0) {
                // The oracle halted the loop at the top of iteration `at` (src/cutting_plane.rs:216-219), before that
                // iteration's commit, which would have carried the shrink of the cut before it: that cut's update is
                // complete in the reference.  Its gt is still in its slot and DevState still holds its scalars (every
                // scalar stage since was a no-op).  (at == 0: the previous batch's closing commit has applied it.)
                if (at >= nb) return fail(ELLHIP_E_STATE, "device loop: inconsistent iteration count");
                s->cur = slot_of[(size_t)(at - 1)];
                rc = do_commit(s, true, nullptr);
                if (rc) return rc;
            }
            HIPCHK(hipStreamSynchronize(st));
        }
        done += nb;
    }
    drop_prime(s);
    rc = read_back(s);
    if (rc) return rc;
    rc = stage.finish(st, stopped ? s->h_result->niter : max_iters);
    if (rc) return rc;
    // plain queues and direct updates do not test a tolerance
    s->h_result->tol = -1.0;
    s->h_result->stop = STOP_NONE;
    s->h_result->niter = 0;
    HIPCHK(hipMemcpyAsync(s->d_st, s->h_result, sizeof(DevState), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace
