// ell_queue_capi.inc.hpp -- the device-resident cut queue cut by cut (queue_prime_impl / queue_cut_impl / queue_commit_impl)
// and the overlapped run that issues the next cut's GEMV ahead on the second stream (queue_run_overlapped).
// Needs: ell_primitives_capi.inc.hpp, ell_side_capi.inc.hpp.  DESIGN.md section 3.6.

namespace {

void queue_free(ellhip_space* s) {
    s->mem.free(s->d_qparams);
    s->mem.free(s->d_qgrads);
    s->mem.free(s->d_qstatus);
    s->mem.free(s->d_qtsq);
    s->qk = 0;
}

const double* qgrad(const ellhip_space* s, long long i) { return s->d_qgrads + (size_t)i * (size_t)s->n; }

int queue_index_ok(const ellhip_space* s, long long i) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (i < 0 || i >= s->qk) return fail(ELLHIP_E_INVALID, "queue index out of range");
    return 0;
}

// queue: make sure gt[cur] = Q * grad[index] (no-op when the previous commit already fused it)
int queue_prime_impl(ellhip_space* s, long long index) {
    if (s->primed && s->primed_qindex == index) return 0;
    int rc = ensure_committed(s);
    if (rc) return rc;
    rc = do_prime(s, qgrad(s, index), s->cur);
    if (rc) return rc;
    s->primed = true;
    s->g_cur = qgrad(s, index);
    s->primed_qindex = index;
    return 0;
}

int queue_cut_impl(ellhip_space* s, long long index) {
    if (!(s->primed && s->primed_qindex == index)) return fail(ELLHIP_E_STATE, "queue_cut: this cut is not primed");
    CutParams none{};
    int rc = do_cut(s, s->g_cur, s->d_qparams + index, none, 1, s->d_qstatus + index, s->d_qtsq + index);
    if (rc) return rc;
    s->shrink_pending = true;  // whether it really applies is decided on the device (DevState.apply)
    s->scalars_stale = true;   // kappa / tsq now live on the device until the next read-back
    return 0;
}

int queue_commit_impl(ellhip_space* s, long long index, long long next) {
    (void)index;
    const double* gnext = (next >= 0) ? qgrad(s, next) : nullptr;
    int rc = do_commit(s, s->shrink_pending, gnext);
    if (rc) return rc;
    s->shrink_pending = false;
    if (gnext) {
        s->cur ^= 1;
        s->primed = true;
        s->g_cur = gnext;
        s->primed_qindex = next;
    } else {
        drop_prime(s);
    }
    return 0;
}

// ---- pipelined queue runs with the next GEMV issued ahead (ELLHIP_OPT_OVERLAP) ---------------------------------------
// On the recorded schedule y = Q_base * g of the NEXT queued cut does not depend on the cut being taken (Q_base only
// changes in an apply pass; the scalar stage corrects y with the recorded updates afterwards), and the queue holds the
// next gradient already.  So k_symv of cut i+1 goes to a second, low-priority stream BEFORE the scalar stage of cut i is
// enqueued, into the other set of partial sums; its reduction (which also forms the dot products with the vector cut i
// records) follows on the main stream once both are done.  The 27 us of reduction + scalar stage per cut then run beside
// the 190 us GEMV instead of between two of them.  Same kernels, same operands, same order of every sum: bit-identical
// to the serial issue order.  Not across an apply pass (the GEMV after it reads the matrix it writes), not on shards
// (their collective sits between the GEMV and the scalar stage), not while profiling events would be recorded out of
// order -- ProfScope takes the stream a kernel is launched on.
bool overlap_ok(const ellhip_space* s) {
    return s->overlap && s->variant == ELLHIP_SPACE_ELL && !s->sharded && symv_ok(s);
}

int overlap_setup(ellhip_space* s) {
    if (s->d_rowpart2) return 0;
    int rc = side_setup(s);
    if (rc) return rc;
    return part_pair_alloc(s, s->d_rowpart2, s->d_colpart2, rowpart_elems(s) * sizeof(double), colpart_elems(s) * sizeof(double));
}

int queue_run_overlapped(ellhip_space* s, long long first, long long count) {
    int rc = overlap_setup(s);
    if (rc) return rc;
    SideGuard guard{s};
    for (long long i = first; i < first + count; ++i) {
        rc = queue_prime_impl(s, i);  // (only the first cut of a run pays its GEMV on the main stream)
        if (rc) return rc;
        const long long next = (i + 1 < s->qk) ? i + 1 : -1;
        // this cut becomes recorded update number npend; when that fills the slots an apply pass follows it, and the
        // next GEMV has to read what that pass writes
        const bool ahead = next >= 0 && symv_ok(s) && s->npend + 1 < s->defer;
        const int set = s->part_set ^ 1;
        if (ahead) {
            rc = side_fork(s);
            if (!rc) rc = launch_symv_tiles(s, qgrad(s, next), side_stream(s), set);
            if (!rc) rc = side_mark(s);
            if (rc) return rc;
        }
        rc = queue_cut_impl(s, i);
        if (rc) return rc;
        if (!ahead) {
            rc = queue_commit_impl(s, i, next);  // apply pass if due, then GEMV + reduction on the main stream
            if (rc) return rc;
            continue;
        }
        // what queue_commit_impl does on this schedule when no apply pass is due, with the GEMV already in flight
        s->shrink_pending = false;
        s->dots_np = 0;
        s->dots_need_gy = false;
        rc = side_join(s);
        if (rc) return rc;
        s->part_set = set;
        rc = launch_symv_reduce(s, qgrad(s, next), s->d_gt[s->cur ^ 1]);
        if (rc) return rc;
        s->cur ^= 1;
        s->primed = true;
        s->g_cur = qgrad(s, next);
        s->primed_qindex = next;
    }
    return 0;
}

}  // namespace
