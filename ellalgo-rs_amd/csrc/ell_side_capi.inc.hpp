// ell_side_capi.inc.hpp -- the second stream of the queue runs: side_setup, side_fork / side_mark / side_join and SideGuard.
// Needs: ell_handle_capi.inc.hpp.  Ahead of ell_passes_capi.inc.hpp because every writer of Q there (flush_pending) joins
// first; the runs that fork are in ell_queue_capi.inc.hpp and ell_group_capi.inc.hpp.  DESIGN.md section 3.6.

namespace {

// ---- the second stream: three functions carry every cross-stream ordering of the queue runs -------------------------
// queue_run_overlapped (the next cut's GEMV) and queue_run_multi (the next group's products) issue kernels that READ Q
// and WRITE one half of the partial-sum sets on a second stream beside the handle's own.  The rules:
//   side_fork   what is issued on the second stream from here on follows EVERYTHING enqueued on the handle's stream so
//               far -- whatever wrote Q (apply passes of this loop, of a cut taken by itself, of ensure_committed) and
//               whatever read the half about to be overwritten.  Not "the events that matter": both ordering bugs of
//               round 3 were a writer of Q that one of several hand-placed events did not cover.
//   side_mark   the side kernels have been issued (records their completion event).
//   side_join   the handle's stream waits for them.  Called before their results are read, by every writer of Q on the
//               handle's stream (flush_pending) and when a queue run returns (SideGuard): nothing outside a queue run
//               ever sees side work in flight.
// ELLHIP_OPT_OVERLAP = 2 issues the "side" kernels on the handle's own stream (same kernels, same order of issue, one
// stream): the serial form the option-mix walks compare the overlapped one against, seed by seed.
int side_setup(ellhip_space* s) {
    if (s->symv_stream) return 0;
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_symv, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_side_go, hipEventDisableTiming);
    // lowest priority: the short reduction / scalar kernels of the main stream get the CU slots the GEMV's workgroups free
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&s->symv_stream, hipStreamNonBlocking, least);
    if (e == hipSuccess) return 0;
    if (s->ev_symv) (void)hipEventDestroy(s->ev_symv);  // all three or none (the stream, created last, is the mark)
    if (s->ev_side_go) (void)hipEventDestroy(s->ev_side_go);
    s->ev_symv = s->ev_side_go = nullptr;
    s->symv_stream = nullptr;
    return fail(ELLHIP_E_HIP, "second stream of the queue runs", e);
}
hipStream_t side_stream(const ellhip_space* s) { return s->overlap == 2 ? s->stream : s->symv_stream; }
int side_join(ellhip_space* s) {
    if (!s->side_busy) return 0;
    s->side_busy = false;
    if (side_stream(s) != s->stream) HIPCHK(hipStreamWaitEvent(s->stream, s->ev_symv, 0));
    return 0;
}
int side_fork(ellhip_space* s) {
    int rc = side_join(s);  // (one batch of side work at a time)
    if (rc) return rc;
    if (side_stream(s) != s->stream) {
        HIPCHK(hipEventRecord(s->ev_side_go, s->stream));
        HIPCHK(hipStreamWaitEvent(s->symv_stream, s->ev_side_go, 0));
    }
    return 0;
}
int side_mark(ellhip_space* s) {
    if (side_stream(s) != s->stream) HIPCHK(hipEventRecord(s->ev_symv, side_stream(s)));
    s->side_busy = true;
    return 0;
}
struct SideGuard {  // a queue run never returns (error paths included) with side work in flight
    ellhip_space* s;
    ~SideGuard() { (void)side_join(s); }
};

}  // namespace
