// ell_primitives_capi.inc.hpp -- the three primitives every update is built from (do_prime, do_cut, do_commit), reading the
// state back (read_back; live_publish / live_wait for direct updates), staging a host gradient, making Q current for an
// observer, and a handle's life cycle (alloc_common, write_state, create_impl).
// Needs: ell_passes_capi.inc.hpp (the passes), ellstable_capi.inc.hpp (EllStable's cut is its whole update).
// DESIGN.md sections 3.2, 3.3, 3.7.

namespace {

// ---- the three primitives --------------------------------------------------------------------

// gt[slot] = Q * g  (Ell only; EllStable has no separate first pass)
int do_prime(ellhip_space* s, const double* g_dev, int slot) {
    if (s->variant != ELLHIP_SPACE_ELL) return 0;
    s->dots_np = 0;  // whatever d_partial held belonged to an earlier gradient
    s->dots_need_gy = false;
    if (symv_ok(s)) return launch_symv(s, g_dev, s->d_gt[slot]);
    if (s->shard_symmetric)
        return fail(ELLHIP_E_STATE, "symmetric row shard: only the deferred (depth 8) schedule is available");
    ProfScope ps(s, CLS_GEMV);
    // deferred depth 8 on full rows (no lower-triangle schedule at this size): the dot products ride along.  Up to
    // n = 8192 only: every workgroup of the scalar stage re-forms g.y from all of g and y, which stops paying beyond.
    if (deferring(s) && s->defer == 8 && !s->sharded && s->fuse_dots && s->n <= 8192)
        return launch_gemv_dots(s, g_dev, s->d_gt[slot]);
    return launch_sweep<false, true>(s, s->sh_gemv, nullptr, g_dev, s->d_gt[slot]);
}

// scalar stage of the primed cut (asynchronous; the caller reads the state back if it needs it)
int do_cut(ellhip_space* s, const double* g_dev, const CutParams* cp_dev, CutParams cp_val, int queue_mode, int* qst,
           double* qtsq) {
    s->xc_host_valid = false;  // the scalar stage moves the centre
    if (s->variant != ELLHIP_SPACE_ELL) return ellstable_issue(s, g_dev, cp_dev, cp_val, queue_mode, qst, qtsq);
    // The dot products a prime left in d_partial belong to THIS cut only: whatever path the cut takes (also the
    // non-deferred one, after a depth switch between prime and cut) they are spent now, and a gradient primed later
    // by a fused pass (rank-1 + GEMV, apply + GEMV) has none.
    const int dots_np_now = s->dots_np;
    s->dots_np = 0;
    ProfScope ps(s, CLS_SCALAR);
    EllCalcDev calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    const unsigned G = (unsigned)scalar_groups(s->n);
    const double* gt = s->d_gt[s->cur];
    if (deferring(s)) {
        // gt currently holds y = Q_base * g; the stage corrects it with the pending updates and records the
        // cut as pending update number s->npend (optimistically counted; see ellhip_queue_results / callers)
        // The dot products come from k_symv_reduce when THIS gradient was primed by it at the depth in force
        // (dots_np); any other history (full-row GEMV, a shard, a depth or mode switch since) takes the separate launch.
        const bool have_dots = dots_np_now == s->defer;
        const bool gy_inside = have_dots && s->dots_need_gy;
        const int npart = (have_dots && !gy_inside) ? (int)((s->n + 127) / 128) : (int)G;
        // a live update: the stage's own workgroups push the centre and the state to the host (live_tail) -- no k_publish launch
        LiveMirror* lm = nullptr;
        unsigned long long lseq = 0;
        if (s->live_arm && queue_mode == 0) {
            s->live_seq += 1;
            lm = s->h_live;
            lseq = s->live_seq;
            s->live_done = true;
        }
        auto go = [&](auto npc) {  // k_scalar_dot_def (when no pass left the dot products behind), then k_scalar_apply_def
            constexpr int NP = decltype(npc)::value;
            if (!have_dots)
                hipLaunchKernelGGL(k_scalar_dot_def<NP>, dim3(G), dim3(256), 0, s->stream, s->n, g_dev, gt, (const double*)s->d_pend,
                                   s->d_partial, s->d_st);
            with_bool(gy_inside, [&](auto gy) {  // (the stage forms g.y itself, from g_dev)
                hipLaunchKernelGGL((k_scalar_apply_def<NP, decltype(gy)::value>), dim3(G), dim3(256), 0, s->stream, s->n, gt, s->d_xc,
                                   s->d_pend, s->d_cpend, (const double*)s->d_partial, s->d_st, calc, cp_dev, cp_val, s->npend, queue_mode,
                                   qst, qtsq, npart, gy_inside ? g_dev : (const double*)nullptr, lm, s->h_xc, lseq, s->d_pub_arrived);
            });
        };
        if (!with_int(Ints<8, 16, 24>{}, s->defer, go)) go(std::integral_constant<int, 8>{});
        HIPCHK(hipGetLastError());
        s->npend += 1;
        return 0;
    }
    if (s->n < SCALAR_SPLIT_N) {
        hipLaunchKernelGGL(k_scalar, dim3(1), dim3(1024), 0, s->stream, s->n, g_dev, gt, s->d_xc, s->d_st, calc,
                           cp_dev, cp_val, s->no_defer_trick, queue_mode, qst, qtsq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(k_scalar_dot, dim3(G), dim3(256), 0, s->stream, s->n, g_dev, gt, s->d_partial, s->d_st);
    hipLaunchKernelGGL(k_scalar_apply, dim3(G), dim3(256), 0, s->stream, s->n, gt, s->d_xc,
                       (const double*)s->d_partial, s->d_st, calc, cp_dev, cp_val, s->no_defer_trick, queue_mode,
                       qst, qtsq);
    HIPCHK(hipGetLastError());
    return 0;
}

// rank-1 pass for the cut just taken (the kernel itself skips it when the cut failed), fused with
// the GEMV pass of `gnext_dev` (into the other slot) when that is given.
int do_commit(ellhip_space* s, bool shrink, const double* gnext_dev) {
    if (s->variant != ELLHIP_SPACE_ELL) return 0;
    if (deferring(s)) {
        // nothing to shrink now: the cut was recorded.  When the slots are full, one pass applies them all
        // (and carries the next GEMV); otherwise the next gradient only needs a read-only pass.
        if (s->npend >= s->defer) {
            if (gnext_dev && !symv_ok(s)) return flush_pending(s, gnext_dev, s->d_gt[s->cur ^ 1]);
            int rc = flush_pending(s, nullptr, nullptr);  // the next GEMV runs on the lower triangle afterwards
            if (rc) return rc;
        }
        if (gnext_dev) return do_prime(s, gnext_dev, s->cur ^ 1);
        return 0;
    }
    if (shrink) {
        int rc = launch_mirror_if_needed(s);
        if (rc) return rc;
    }
    const double* gt_cur = s->d_gt[s->cur];
    if (shrink && gnext_dev) {
        ProfScope ps(s, CLS_FUSED);
        return launch_sweep<true, true>(s, s->sh_fused, gt_cur, gnext_dev, s->d_gt[s->cur ^ 1]);
    }
    if (shrink) {
        ProfScope ps(s, CLS_RANK1);
        return launch_sweep<true, false>(s, s->sh_rank1, gt_cur, nullptr, nullptr);
    }
    if (gnext_dev) return do_prime(s, gnext_dev, s->cur ^ 1);
    return 0;
}

int read_back(ellhip_space* s) {
    HIPCHK(hipMemcpyAsync(s->h_result, s->d_st, sizeof(DevState), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->kappa = s->h_result->kappa;
    s->tsq = s->h_result->tsq;
    s->scalars_stale = false;
    if (s->h_result->solve_err) {
        // A bounded wait of a persistent solve gave up: this update's result is invalid and the call fails.  The
        // error word is cleared once it has been reported and the handle falls back to one launch per block (no
        // inter-workgroup waits), so the handle stays usable -- its state, though, is what the failed update left.
        // (Ell: resident batches settle their own time-outs inside resident_run and leave no error word behind.)
        s->h_result->solve_err = 0;
        (void)hipMemsetAsync(reinterpret_cast<char*>(s->d_st) + offsetof(DevState, solve_err), 0, sizeof(int), s->stream);
        (void)hipStreamSynchronize(s->stream);
        if (s->variant == ELLHIP_SPACE_ELL) {
            s->resident = 0;
            return fail(ELLHIP_E_HIP, "a bounded in-launch wait timed out on an Ell handle; resident batches are now off on it");
        }
        s->stable_solve = 0;
        (void)stable_mirror_leave(s);  // (flags only matter from here on: the buffer is what the failed update left)
        return fail(ELLHIP_E_HIP, "a bounded in-launch wait of an EllStable persistent solve timed out; this handle now uses one "
                                  "launch per block (no inter-workgroup waits)");
    }
    return 0;
}

// ---- live updates: what the caller's next statement needs, and no more ---------------------------------------------
// live_publish is enqueued right behind the scalar stage of a direct update; live_wait returns as soon as that update's
// status / tsq / kappa and the new centre are in host memory.  Whatever the update still has in flight behind it (the
// rank-1 pass, an apply pass of the recorded schedule) keeps running: the next call on the handle is ordered after it by
// the stream.  Same observable contract as read_back (h_result, kappa, tsq, the solve_err protocol).
int live_publish(ellhip_space* s) {
    if (s->live_done) {   // the scalar stage has published itself (live_tail)
        s->live_done = false;
        return 0;
    }
    s->live_seq += 1;
    const unsigned wgs = (unsigned)std::max<long long>(1, std::min<long long>(PUB_WGS, s->n / 1024));
    hipLaunchKernelGGL(k_publish, dim3(wgs), dim3(256), 0, s->stream, (const DevState*)s->d_st, (const double*)s->d_xc, s->n,
                       s->h_live, s->h_xc, s->live_seq, s->d_pub_arrived);
    HIPCHK(hipGetLastError());
    return 0;
}
int live_wait(ellhip_space* s) {
    const unsigned long long want = s->live_seq;
    const unsigned long long* seq = &s->h_live->seq;
    for (unsigned spin = 1;; ++spin) {
        if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == want) break;
        if ((spin & 0x3fffu) == 0) {  // now and then: is the stream still alive?
            const hipError_t q = hipStreamQuery(s->stream);
            if (q == hipSuccess) {    // drained: the word must be there
                if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == want) break;
                return fail(ELLHIP_E_HIP, "live update: the stream drained without publishing its result");
            }
            if (q != hipErrorNotReady) return fail(ELLHIP_E_HIP, "live update", q);
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    *s->h_result = s->h_live->st;
    s->kappa = s->h_result->kappa;
    s->tsq = s->h_result->tsq;
    s->scalars_stale = false;
    s->xc_host_valid = true;
    if (s->h_result->solve_err) return read_back(s);  // (rare: the full protocol, with the stream drained)
    return 0;
}

// upload a host gradient into stage slot `slot`
int stage_grad(ellhip_space* s, const double* grad, int slot) {
    if (!grad) return fail(ELLHIP_E_INVALID, "grad is NULL");
    const size_t bytes = (size_t)s->n * sizeof(double);
    if (s->stage_direct) {
        // Nothing in flight reads this slot: every reader of a staged gradient (the GEMV, the scalar stage, EllStable's forward
        // solve) has finished before the call that consumed it returned, and the other slot is the one a primed gradient holds.
        memcpy(s->d_stage[slot], grad, bytes);
        __atomic_thread_fence(__ATOMIC_SEQ_CST);   // (write-combined stores drained before the launch's doorbell)
        return 0;
    }
    memcpy(s->h_stage[slot], grad, bytes);
    // (the chip pulls the staging buffer over PCIe itself: no copy engine, no cross-engine hand-over in front of the GEMV)
    const unsigned wgs = (unsigned)std::max<long long>(1, std::min<long long>(STAGE_WGS, s->n / 512));
    hipLaunchKernelGGL(k_stage, dim3(wgs), dim3(256), 0, s->stream, (const double*)s->h_stage[slot], s->d_stage[slot], s->n);
    HIPCHK(hipGetLastError());
    return 0;
}

int make_params(int kind, double b0, int has_b1, double b1, CutParams& cp) {
    if (kind < 0 || kind > 2) return fail(ELLHIP_E_INVALID, "bad cut kind");
    cp.kind = kind;
    cp.has_b1 = has_b1 ? 1 : 0;
    cp.b0 = b0;
    cp.b1 = has_b1 ? b1 : 0.0;
    return 0;
}

// Make Q current: issue a shrink that a previous ellhip_cut / queue cut left pending.
int ensure_committed(ellhip_space* s) {
    if (s->in_two_phase) return fail(ELLHIP_E_STATE, "update_begin without update_end");
    if (s->shrink_pending) {
        int rc = do_commit(s, true, nullptr);
        if (rc) return rc;
        s->shrink_pending = false;
    }
    return 0;
}

void drop_prime(ellhip_space* s) {
    s->primed = false;
    s->g_cur = nullptr;
    s->primed_qindex = -1;
}

// A gradient that is primed but not yet cut carries y = Q_base * g for the base the recorded updates belong to
// (the scalar stage corrects it with them).  When something other than the cut sequence itself applies the
// recorded updates -- ellhip_flush, or an observer of Q between commit(next) and cut(next) -- the base changes
// under that y, so it is recomputed against the new base.  A row shard cannot (its GEMV needs the owner's
// collective): its prime is dropped instead and the owner primes again (ellhip_queue_primed tells).
bool prime_is_uncut(const ellhip_space* s) {
    return s->variant == ELLHIP_SPACE_ELL && s->primed && !s->shrink_pending && s->g_cur != nullptr;
}
int refresh_prime(ellhip_space* s) {
    if (s->sharded) {
        drop_prime(s);
        return 0;
    }
    return do_prime(s, s->g_cur, s->cur);
}

// For observers of Q itself (get_mq, clone, mode switches): also apply what deferred mode has recorded.
int make_q_current(ellhip_space* s) {
    if (s->variant == ELLHIP_SPACE_ELL_STABLE) {  // (the buffer in the reference's layout)
        const int erc = ensure_committed(s);
        return erc ? erc : stable_mirror_leave(s);
    }
    const bool uncut = prime_is_uncut(s);
    int rc = ensure_committed(s);
    if (rc) return rc;
    if (s->npend > 0) {
        rc = flush_pending(s, nullptr, nullptr);
        if (rc) return rc;
        if (uncut) {
            rc = refresh_prime(s);
            if (rc) return rc;
        }
    }
    if (s->upper_stale && !s->sharded) {  // lower-triangle-only apply passes ran: rebuild the mirrored half
        // (a symmetric row shard cannot: the mirrored elements live on other ranks; its rows stay valid up to
        // their diagonal only, see ellhip_set_shard_symmetric)
        const unsigned t = (unsigned)((s->n + 31) / 32);
        hipLaunchKernelGGL(k_mirror_lower_now, dim3(t, t), dim3(256), 0, s->stream, s->d_Q, s->ld, s->n);
        HIPCHK(hipGetLastError());
        s->upper_stale = false;
    }
    return 0;
}

int alloc_common(ellhip_space* s) {
    const long long n = s->n;
    const size_t vbytes = (size_t)n * sizeof(double);
    HIPCHK(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    s->stream = s->own_stream;
    HIPCHK(s->mem.device(s->d_Q, (size_t)s->nrows * (size_t)s->ld * sizeof(double)));
    HIPCHK(s->mem.device(s->d_xc, vbytes));
    {   // Large-BAR systems: the host writes a gradient straight into device memory (fine-grained allocation: 3 us for 128 KiB)
        // instead of into a pinned buffer that a kernel then pulls over PCIe (0.8 + 7.6 us and a launch on the live loop's
        // critical path, tools/experiments/bar_write.hip).
        int large_bar = 0;
        if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, s->device) != hipSuccess) large_bar = 0;
        (void)hipGetLastError();
        s->stage_direct = large_bar != 0 && g_defaults.stage_direct != 0;
    }
    if (s->stage_direct) {
        const size_t mark = s->mem.mark();
        for (int k = 0; k < 2 && s->stage_direct; ++k)
            if (s->mem.device_finegrained(s->d_stage[k], vbytes) != hipSuccess) {
                (void)hipGetLastError();
                s->mem.rollback(mark);
                s->stage_direct = false;
            }
    }
    if (!s->stage_direct)
        for (int k = 0; k < 2; ++k) HIPCHK(s->mem.device(s->d_stage[k], vbytes));
    for (int k = 0; k < 2; ++k) {
        HIPCHK(s->mem.device(s->d_gt_own[k], vbytes));
        s->d_gt[k] = s->d_gt_own[k];
        HIPCHK(s->mem.pinned(s->h_stage[k], vbytes, hipHostMallocCoherent | hipHostMallocMapped));  // (k_stage reads it from the device)
        HIPCHK(hipMemsetAsync(s->d_gt_own[k], 0, vbytes, s->stream));
    }
    HIPCHK(s->mem.device(s->d_st, sizeof(DevState)));
    // partial sums of the scalar stage: [scalar_groups(n) <= 64][MAXPEND + 1], or [ceil(n / 128)][depth + 1] when the
    // lower-triangle GEMV's reduction produces them
    HIPCHK(s->mem.device(s->d_partial, (size_t)std::max<long long>(64, (n + 127) / 128) * (MAXPEND + 1) * sizeof(double)));
    if (s->variant == ELLHIP_SPACE_ELL) {
        HIPCHK(s->mem.device(s->d_pend, (size_t)MAXPEND * vbytes));
        HIPCHK(s->mem.device(s->d_cpend, MAXPEND * sizeof(double)));
        HIPCHK(hipMemsetAsync(s->d_pend, 0, (size_t)MAXPEND * vbytes, s->stream));
        HIPCHK(hipMemsetAsync(s->d_cpend, 0, MAXPEND * sizeof(double), s->stream));
    }
    if (s->variant == ELLHIP_SPACE_ELL_STABLE) {
        const size_t nflags = (size_t)std::max<long long>(512, (n + SB - 1) / SB);
        HIPCHK(s->mem.device(s->d_flags, nflags * sizeof(int)));
        HIPCHK(hipMemsetAsync(s->d_flags, 0, nflags * sizeof(int), s->stream));
        {   // how many workgroups of each persistent solve this device keeps resident at once
            hipDeviceProp_t prop;
            HIPCHK(hipGetDeviceProperties(&prop, s->device));
            auto cap = [&](const void* fwd, const void* bwd, int threads) -> int {
                int a = 0, b = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, fwd, threads, 0) != hipSuccess) a = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, bwd, threads, 0) != hipSuccess) b = 0;
                return std::min(a, b) * prop.multiProcessorCount;
            };
            s->persist_cap1 = cap((const void*)k_st_fwd_persist, (const void*)k_st_bwd_persist, 256);
            s->persist_cap_h = std::min(cap((const void*)k_st_fwd_helped<false>, (const void*)k_st_bwd_factor_helped<2048, 8>, 256),
                                        cap((const void*)k_st_fwd_helped<true>, (const void*)k_st_bwd_factor_helped<2048, 8, true>, 256));
        }
        {   // the 16-row factor tiles of k_st_bwd_factor_helped: the active tiles of the strict upper triangle, full ones first
            const long long seg = (n >= 8192) ? 2048 : 512;
            const long long nseg = (n + seg - 1) / seg;
            std::vector<int> f16, e16;
            const long long ngrp = (n + FQ_H - 1) / FQ_H;
            for (long long I = 0; I < ngrp && nseg <= 16; ++I)
                for (long long J = 0; J < nseg; ++J) {
                    const long long r0 = I * FQ_H, c0 = J * seg;
                    if (c0 + seg - 1 <= r0) continue;
                    const long long rlast = std::min(r0 + FQ_H - 1, n - 1);
                    ((c0 > rlast && c0 + seg <= n) ? f16 : e16).push_back((int)((I << 4) | J));
                }
            f16.insert(f16.end(), e16.begin(), e16.end());
            s->nftiles16 = (int)f16.size();
            HIPCHK(s->mem.device(s->d_fnext, sizeof(int)));
            HIPCHK(hipMemsetAsync(s->d_fnext, 0, sizeof(int), s->stream));
            if (s->nftiles16 > 0) {
                HIPCHK(s->mem.device(s->d_ftiles16, f16.size() * sizeof(int)));
                HIPCHK(hipMemcpyAsync(s->d_ftiles16, f16.data(), f16.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
                HIPCHK(hipStreamSynchronize(s->stream));  // `f16` goes out of scope
                HIPCHK(s->mem.device(s->d_qhpart, vbytes));
                hipLaunchKernelGGL(k_st_arm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->d_qhpart, n);
            }
        }
        HIPCHK(hipStreamCreateWithFlags(&s->aux_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
        HIPCHK(s->mem.device(s->d_work, vbytes * 8 + (ST_MID_T + 8) * sizeof(double)));  // w0 z gg q beta2 qpub w1 (+1 spare) | cpre
        // both publish buffers of the persistent forward solve start out all-sentinel
        hipLaunchKernelGGL(k_st_arm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->d_work, n);
        hipLaunchKernelGGL(k_st_arm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->d_work + 6 * n, n);
        HIPCHK(s->mem.device(s->d_hpart, vbytes));
        hipLaunchKernelGGL(k_st_arm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->d_hpart, n);
        HIPCHK(s->mem.device(s->d_stpend, sizeof(StPend)));
        HIPCHK(s->mem.device(s->d_rbuf, 2 * vbytes));
        HIPCHK(s->mem.device(s->d_wkeep, vbytes));
        hipLaunchKernelGGL(k_st_mirror_clear, dim3(1), dim3(1), 0, s->stream, s->d_stpend);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(s->mem.pinned(s->h_result, sizeof(DevState), hipHostMallocDefault));
    HIPCHK(s->mem.pinned(s->h_live, sizeof(LiveMirror), hipHostMallocCoherent | hipHostMallocMapped));
    HIPCHK(s->mem.pinned(s->h_xc, vbytes, hipHostMallocCoherent | hipHostMallocMapped));
    memset(s->h_live, 0, sizeof(LiveMirror));
    HIPCHK(s->mem.device(s->d_pub_arrived, sizeof(unsigned)));
    HIPCHK(hipMemsetAsync(s->d_pub_arrived, 0, sizeof(unsigned), s->stream));
    return 0;
}

int write_state(ellhip_space* s) {
    DevState st;
    memset(&st, 0, sizeof st);
    st.kappa = s->kappa;
    st.tsq = s->tsq;
    st.scale = 1.0;
    st.status = ELLHIP_SUCCESS;
    st.tol = -1.0;
    *s->h_result = st;
    HIPCHK(hipMemcpyAsync(s->d_st, s->h_result, sizeof(DevState), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

// Bitwise symmetry test of the caller's matrix, in 64 x 64 tiles so that the transposed accesses stay in cache
// (a plain double loop walks one operand with stride n: tens of seconds at n = 16384).
bool host_is_symmetric(const double* mq, long long n) {
    constexpr long long T = 64;
    for (long long i0 = 0; i0 < n; i0 += T)
        for (long long j0 = 0; j0 <= i0; j0 += T) {
            const long long i1 = std::min(i0 + T, n), j1 = std::min(j0 + T, n);
            for (long long i = i0; i < i1; ++i)
                for (long long j = j0; j < j1 && j < i; ++j)
                    if (memcmp(&mq[i * n + j], &mq[j * n + i], sizeof(double)) != 0) return false;
        }
    return true;
}

int create_impl(ellhip_space** out, int variant, long long n, long long row0, long long nrows, bool sharded,
                double kappa, const double* mq, const double* diag, const double* xc, int device) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1 || nrows < 1 || row0 < 0 || row0 + nrows > n) return fail(ELLHIP_E_INVALID, "bad dimensions");
    if (variant != ELLHIP_SPACE_ELL && variant != ELLHIP_SPACE_ELL_STABLE)
        return fail(ELLHIP_E_INVALID, "unknown variant");
    if (sharded && variant != ELLHIP_SPACE_ELL)
        return fail(ELLHIP_E_INVALID, "EllStable does not shard (replicas only)");
    int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the ellipsoid engine has no CPU path");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");

    ellhip_space* s = new (std::nothrow) ellhip_space();
    if (!s) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    s->variant = variant;
    s->n = n;
    s->row0 = row0;
    s->nrows = nrows;
    s->sharded = sharded;
    s->device = device;
    s->kappa = kappa;
    s->tsq = 0.0;
    // Leading dimension: rows stay 16-byte aligned for even n.  For blocks that stream from HBM a
    // power-of-two row pitch is broken up with one extra 128-byte line per row (GEMV pass at
    // n = 16384: 5.8 -> 6.3 TB/s); blocks that live in the Infinity Cache are left dense.
    s->ld = n;
    if ((n % 512) == 0 && (double)nrows * (double)n * 8.0 > 200.0 * 1024 * 1024) s->ld = n + 16;
    if (g_defaults.pad >= 0) s->ld = n + g_defaults.pad;  // ELLHIP_OPT_PAD (tuning runs)
    if ((n % 2) == 0 && (s->ld % 2) != 0) s->ld += 1;
    if (variant == ELLHIP_SPACE_ELL_STABLE) s->ld = n + (n & 1);  // 16-byte aligned rows for the 2-column lanes
    pick_shape(s);

    DeviceGuard guard(device);
    int rc = alloc_common(s);
    if (rc) {
        ellhip_destroy(s);
        return rc;
    }
    auto bail = [&](int code) {
        ellhip_destroy(s);
        return code;
    };
    // centre
    if (xc) {
        memcpy(s->h_stage[0], xc, (size_t)n * sizeof(double));
        if (hipMemcpyAsync(s->d_xc, s->h_stage[0], (size_t)n * sizeof(double), hipMemcpyHostToDevice, s->stream) !=
            hipSuccess)
            return bail(fail(ELLHIP_E_HIP, "upload xc"));
        if (hipStreamSynchronize(s->stream) != hipSuccess) return bail(fail(ELLHIP_E_HIP, "sync"));
    } else {
        if (hipMemsetAsync(s->d_xc, 0, (size_t)n * sizeof(double), s->stream) != hipSuccess)
            return bail(fail(ELLHIP_E_HIP, "memset xc"));
    }
    // matrix
    if (mq) {
        if (hipMemcpy2DAsync(s->d_Q, (size_t)s->ld * sizeof(double), mq, (size_t)n * sizeof(double),
                             (size_t)n * sizeof(double), (size_t)nrows, hipMemcpyHostToDevice,
                             s->stream) != hipSuccess)
            return bail(fail(ELLHIP_E_HIP, "upload mq"));
        if (s->ld != n) {
            // zero the padding columns so they never hold NaNs
            if (hipMemset2DAsync(s->d_Q + n, (size_t)s->ld * sizeof(double), 0, (size_t)(s->ld - n) * sizeof(double),
                                 (size_t)nrows, s->stream) != hipSuccess)
                return bail(fail(ELLHIP_E_HIP, "memset pad"));
        }
        if (variant == ELLHIP_SPACE_ELL && !sharded) s->needs_mirror = !host_is_symmetric(mq, n);
    } else {
        double* d_diag = nullptr;
        if (diag) {
            memcpy(s->h_stage[0], diag, (size_t)n * sizeof(double));
            if (hipMemcpyAsync(s->d_stage[0], s->h_stage[0], (size_t)n * sizeof(double), hipMemcpyHostToDevice,
                               s->stream) != hipSuccess)
                return bail(fail(ELLHIP_E_HIP, "upload diag"));
            d_diag = s->d_stage[0];
        }
        hipLaunchKernelGGL(k_fill_diag, dim3(2048), dim3(256), 0, s->stream, s->d_Q, s->ld, n, nrows, row0,
                           (const double*)d_diag);
        if (hipGetLastError() != hipSuccess) return bail(fail(ELLHIP_E_HIP, "k_fill_diag"));
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess) return bail(fail(ELLHIP_E_HIP, "sync after upload"));
    rc = write_state(s);
    if (rc) return bail(rc);
    // Default schedule of a new unsharded Ell handle: depth 24 wherever the lower-triangle schedule exists (even
    // n >= 5120 (ELLHIP_OPT_SYMV_MIN_N): 4.33 n^2 instead of 24 n^2 bytes per update, the recorded updates applied as one rank-24 update on the
    // matrix cores; results within the parity tolerance of depth 1, Q made current for every observer), otherwise the
    // reference's data flow (depth 1).  ELLHIP_OPT_AUTO_DEFER = 0 keeps depth 1 everywhere; ellhip_set_defer_depth overrides either way.  Row shards stay at 1 until their owner chooses.
    // Between 3072 and that size (and for odd n) depth 8 with full-row GEMVs is the faster one, for synchronous calls
    // and for queues alike (tools/depth_sweep.py: n = 4096: 15 800 vs 10 400 calls/s; below ~3000 depth 1 wins).
    if (variant == ELLHIP_SPACE_ELL && !sharded && g_defaults.auto_defer) {
        const bool lower = s->symv && s->apply_lower && (n % 2) == 0 && n >= s->symv_min_n;
        const int depth = lower ? 24 : (n >= 3072 ? 8 : 1);
        if (depth != 1) {
            rc = ellhip_set_defer_depth(s, depth);
            if (rc) return bail(rc);
        }
    }
    *out = s;
    return 0;
}

}  // namespace
