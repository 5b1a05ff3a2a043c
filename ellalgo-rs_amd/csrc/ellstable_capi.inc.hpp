// ellstable_capi.inc.hpp -- EllStable's update as a fixed sequence of launches (ellstable_issue), entering and leaving the
// mirrored layout, and the co-residency token (CoresToken / CoresScope) that chains every launch whose workgroups wait for
// one another: EllStable's persistent solves here, the resident batches in ell_resident_capi.inc.hpp.
// Needs: ell_handle_capi.inc.hpp, launch_dispatch.hpp.  DESIGN.md sections 4, 4.1, 4.2 (the token: 3.5).

namespace {

// ---- one co-residency grid at a time per device ------------------------------------------------------------------------
// Two kinds of launches here consist of workgroups that WAIT for one another inside the launch and therefore assume all of
// them are on the device at once: a resident batch (k_ell_resident, one grid barrier per cut) and EllStable's persistent solves
// (chain / helper workgroups).  Two such grids at the same time -- two handles, two host threads -- can each hold part of the
// CUs and wait for workgroups of its own that the other keeps out: nothing hangs (every wait is bounded) but both time out.
// So within this process they are chained per device: whoever issues one waits, ON THE DEVICE, for the event the previous one
// left behind (hipStreamWaitEvent: no host synchronisation), and leaves its own.  Kernels that merely run long (the
// matrix-core passes draw tiles from a queue and keep their CUs for a whole pass) delay such a grid, they cannot lock it.
constexpr int CORES_MAX_DEVICES = 16;
constexpr int CORES_RING = 64;
struct CoresToken {
    std::mutex m;
    hipEvent_t ring[CORES_RING] = {};
    unsigned next = 0;
    hipEvent_t last = nullptr;
};
CoresToken g_cores[CORES_MAX_DEVICES];

struct CoresScope {  // from before the first such launch of an API call until after the last one has been enqueued
    CoresToken* t;
    hipStream_t stream;
    CoresScope(ellhip_space* s) : t(&g_cores[s->device & (CORES_MAX_DEVICES - 1)]), stream(s->stream) {
        t->m.lock();
        if (t->last) (void)hipStreamWaitEvent(stream, t->last, 0);
    }
    ~CoresScope() {
        hipEvent_t& e = t->ring[t->next % CORES_RING];
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
        if (e && hipEventRecord(e, stream) == hipSuccess) {
            t->last = e;
            t->next += 1;
        }
        t->m.unlock();
    }
    CoresScope(const CoresScope&) = delete;
    CoresScope& operator=(const CoresScope&) = delete;
};

// EllStable, mirrored layout (ELLHIP_OPT_STABLE_SOLVE = 3; ellstable_kernels.hpp, StPend): entering copies the factor below
// the diagonal and sets every row scale to 1 (one 8 n^2-byte pass); leaving -- before anything observes the buffer (get_mq,
// clone), on a mode switch, when a halted queue's results are read, and every ST_MIRROR_PERIOD updates so that the running
// scales stay products of few factors -- rebuilds the scratch triangle of the last forward solve and scales U: the buffer is
// then what the eager kernels leave (to rounding: one rounding per element where they had two per update).
constexpr int ST_MIRROR_PERIOD = 256;
int stable_mirror_enter(ellhip_space* s) {
    const unsigned t = (unsigned)((s->n + 63) / 64);
    hipLaunchKernelGGL(k_st_mirror_enter, dim3(t, t), dim3(256), 0, s->stream, s->d_Q, s->ld, s->n, (const DevState*)s->d_st,
                       s->d_rbuf);
    hipLaunchKernelGGL(k_st_mirror_mark, dim3(1), dim3(1), 0, s->stream, s->d_stpend, (const DevState*)s->d_st);
    HIPCHK(hipGetLastError());
    s->st_mirrored = true;
    s->st_since_enter = 0;
    return 0;
}
int stable_mirror_leave(ellhip_space* s) {
    if (!s->st_mirrored) return 0;
    const long long n = s->n;
    const unsigned t = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(k_st_mirror_leave, dim3(t, t), dim3(256), 0, s->stream, s->d_Q, s->ld, n, (const StPend*)s->d_stpend,
                       (const double*)s->d_rbuf, (const double*)s->d_wkeep);
    hipLaunchKernelGGL(k_st_unscale_upper, dim3((unsigned)std::min<long long>(16, (n + 255) / 256), (unsigned)n), dim3(256), 0,
                       s->stream, s->d_Q, s->ld, n, (const StPend*)s->d_stpend, (const double*)s->d_rbuf);
    hipLaunchKernelGGL(k_st_mirror_clear, dim3(1), dim3(1), 0, s->stream, s->d_stpend);
    HIPCHK(hipGetLastError());
    s->st_mirrored = false;
    return 0;
}

// EllStable::update_core as a fixed sequence of launches (ellstable_kernels.hpp).
int ellstable_issue(ellhip_space* s, const double* g_dev, const CutParams* cp_dev, CutParams cp_val, int queue_mode,
                    int* qst, double* qtsq) {
    const long long n = s->n, ld = s->ld;
    const long long nb = (n + SB - 1) / SB;
    double* w0 = s->d_work;
    double* z = w0 + n;
    double* gg = z + n;
    double* q = gg + n;
    double* beta2 = q + n;
    double* qpub = beta2 + n;            // publish buffer of the persistent backward solve (data-as-flag hand-off)
    double* w1 = qpub + n;               // second publish buffer of the persistent forward solve (see below)
    double* cpre = w1 + n + (n & 1);     // chunk prefixes of the mid stage (ST_MID_T + 1 doubles)
    hipStream_t st = s->stream;
    // One launch per solve when every workgroup of the chain can be resident at once (a workgroup that waits for its
    // predecessor holds its CU: the limit is what the DEVICE holds -- CU count x occupancy of the kernel, measured at
    // handle creation -- not a constant); otherwise one launch per block.
    const bool persist = s->stable_solve >= 1 && nb <= s->persist_cap1;
    // both solves with a helper workgroup per block (two workgroups per block, all resident): k_st_fwd_helped,
    // k_st_bwd_factor_helped (which also pulls the factor tiles)
    const bool helped = persist && s->stable_solve >= 2 && s->d_hpart && 2 * nb <= s->persist_cap_h;
    // Persistent forward solve: the workgroup that is next in the chain polls the VALUES of the block it waits for
    // (sentinel until stored, like the backward solve's qpub), everybody else the block's flag.  The published
    // vector therefore has to be all-sentinel when a solve starts: two buffers alternate by launch parity, and the
    // mid stage of every update re-arms the one the NEXT solve will use (whatever this update's status).
    // (one co-residency grid at a time on the device: chained behind the previous one, CoresScope)
    std::unique_ptr<CoresScope> alone;
    if (persist) alone.reset(new CoresScope(s));
    if (persist) ++s->epoch;
    double* w = (persist && (s->epoch & 1)) ? w1 : w0;
    double* w_next = (persist && (s->epoch & 1)) ? w0 : w1;
    int* err = reinterpret_cast<int*>(reinterpret_cast<char*>(s->d_st) + offsetof(DevState, solve_err));
    // The hand-over buffers of the in-launch waits are re-armed (all-sentinel) by the k_st_post of the update BEFORE the one
    // that polls them.  After a switch of forms (ellhip_set_option between two updates) that update may have run a form that
    // does not: its solve then left real values in w, and a consumer polling "the value is its own flag" would take the old
    // block for the new one.  Arm what this update polls and the previous one did not arm.
    {
        const unsigned ga = (unsigned)((n + 255) / 256);
        if (persist && !s->st_prev_persist) hipLaunchKernelGGL(k_st_arm, dim3(ga), dim3(256), 0, st, w, n);
        if (helped && !s->st_prev_helped) hipLaunchKernelGGL(k_st_arm, dim3(ga), dim3(256), 0, st, s->d_hpart, n);
        s->st_prev_persist = persist;
        s->st_prev_helped = helped;
    }
    // the helped backward solve (with or without factor tiles) needs its tile list / hand-over buffer and both grids resident
    const bool helped_b = helped && s->d_ftiles16 && s->d_fnext && s->d_qhpart && 2 * nb <= s->persist_cap1;
    // the mirrored layout (STABLE_SOLVE = 3): no scratch triangle, no factor pass -- both helped solves in their MIRROR form
    const bool mirror = helped_b && s->stable_solve >= 3 && s->d_stpend;
    // factor update inside the backward solve's launch: needs the helped form and the row-wise (U alone) arithmetic
    const bool fused_h = helped_b && !mirror && s->stable_factor >= 2;
    if (mirror && s->st_mirrored && s->st_since_enter >= ST_MIRROR_PERIOD) {
        int mrc = stable_mirror_leave(s);  // (and in again below: the row scales start from 1)
        if (mrc) return mrc;
    }
    if (mirror != s->st_mirrored) {
        int mrc = mirror ? stable_mirror_enter(s) : stable_mirror_leave(s);
        if (mrc) return mrc;
    }
    if (mirror) s->st_since_enter += 1;
    const StPend* pend_c = mirror ? s->d_stpend : nullptr;
    {
        ProfScope ps(s, CLS_ST_FWD);
        if (helped) {  // (the mirrored layout runs on the helped solves, in their MIRROR form)
            with_bool(mirror, [&](auto m) {
                hipLaunchKernelGGL(k_st_fwd_helped<decltype(m)::value>, dim3((unsigned)(2 * nb)), dim3(256), 0, st, s->d_Q, ld, n, g_dev, w,
                                   s->d_hpart, z, gg, s->d_flags, err, s->epoch, (const DevState*)s->d_st, pend_c,
                                   mirror ? (const double*)s->d_rbuf : (const double*)nullptr);
            });
        } else if (persist) {
            hipLaunchKernelGGL(k_st_fwd_persist, dim3((unsigned)nb), dim3(256), 0, st, s->d_Q, ld, n, g_dev, w, z, gg,
                               s->d_flags, err, s->epoch, s->d_st);
        } else {
            HIPCHK(hipMemcpyAsync(w, g_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(k_st_fwd_first, dim3(1), dim3(256), 0, st, s->d_Q, ld, n, g_dev, w, z, gg, s->d_st);
            for (long long kb = 0; kb + 1 < nb; ++kb) {
                const long long rest = n - (kb + 1) * SB;
                const unsigned grid = (unsigned)((rest + SPANEL - 1) / SPANEL);
                hipLaunchKernelGGL(k_st_fwd_step, dim3(grid), dim3(256), 0, st, s->d_Q, ld, n, kb, w, z, gg, s->d_st);
            }
        }
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(s, CLS_SCALAR);
        EllCalcDev calc = EllCalcDev::make(n, s->use_parallel_cut);
        hipLaunchKernelGGL(k_st_mid, dim3(1), dim3(ST_MID_T), 0, st, n, (const double*)gg, cpre, s->d_st, calc, cp_dev,
                           cp_val, queue_mode, qst, qtsq, mirror ? s->d_stpend : (StPend*)nullptr);
        hipLaunchKernelGGL(k_st_post, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->d_Q, ld, n,
                           (const double*)z, (const double*)gg, (const double*)cpre, q, beta2,
                           persist ? qpub : (double*)nullptr, persist ? w_next : (double*)nullptr,
                           (const DevState*)s->d_st, helped ? s->d_hpart : (double*)nullptr, s->d_fnext,
                           (fused_h || mirror) ? s->d_qhpart : (double*)nullptr, pend_c, s->d_rbuf, (const double*)w, s->d_wkeep);
        HIPCHK(hipGetLastError());
    }
    // The factor update (rewrites U) and the backward solve (reads S, writes q) are independent.  Helped form: the
    // factor tiles are pulled inside the backward solve's launch by whoever is idle.  Otherwise, with the persistent
    // backward solve (latency-bound) the bandwidth-bound factor update runs beside it on the auxiliary stream,
    // launched AFTER it so the solve's workgroups are placed first; the streams join before anything else touches Q.
    const bool overlap = persist && !fused_h && !mirror;
    if (overlap) HIPCHK(hipEventRecord(s->ev_fork, st));
    {
        ProfScope ps(s, CLS_ST_BWD);
        if (mirror) {
            hipLaunchKernelGGL((k_st_bwd_factor_helped<2048, 8, true>), dim3((unsigned)(2 * nb)), dim3(256), 0, st, s->d_Q, ld, n, q,
                               qpub, s->d_qhpart, err, (const DevState*)s->d_st, nb, (const double*)beta2, (const double*)w,
                               (const int*)s->d_ftiles16, s->nftiles16, s->d_fnext, nb + 1, pend_c, (const double*)s->d_rbuf);
        } else if (fused_h) {
            const unsigned grid = (unsigned)(2 * nb);
            // before their turn the chain workgroups pull factor tiles only when the matrix is on-die (n < 8192): from HBM
            // it made them late for their own block (n = 16384: stop distance 6 / 12 / 24 / 48+ blocks: 785 / 731 / 710 /
            // 685-695 us), on-die it pays (n = 4096: 139 us against 170 without)
            const long long fq_stop = n >= 8192 ? nb + 1 : FQ_STOP;
            with_bool(n >= 8192, [&](auto big) {
                hipLaunchKernelGGL((k_st_bwd_factor_helped<decltype(big)::value ? 2048 : 512, 8>), dim3(grid), dim3(256), 0, st, s->d_Q, ld, n,
                                   q, qpub, s->d_qhpart, err, (const DevState*)s->d_st, nb, (const double*)beta2, (const double*)w,
                                   (const int*)s->d_ftiles16, s->nftiles16, s->d_fnext, fq_stop);
            });
        } else if (persist) {
            hipLaunchKernelGGL(k_st_bwd_persist, dim3((unsigned)nb), dim3(256), 0, st, s->d_Q, ld, n, q, qpub, err,
                               s->d_st);
        } else {
            hipLaunchKernelGGL(k_st_bwd_last, dim3(1), dim3(256), 0, st, s->d_Q, ld, n, nb - 1, q, s->d_st);
            for (long long kb = nb - 1; kb >= 1; --kb) {
                const unsigned grid = (unsigned)((kb * SB + SPANEL - 1) / SPANEL);
                hipLaunchKernelGGL(k_st_bwd_step, dim3(grid), dim3(256), 0, st, s->d_Q, ld, n, kb, q, s->d_st);
            }
        }
        const unsigned gx = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(k_st_xc, dim3(gx < 256 ? gx : 256), dim3(256), 0, st, n, q, s->d_xc, s->d_st);
        HIPCHK(hipGetLastError());
    }
    if (!fused_h && !mirror) {
        hipStream_t fs = overlap ? s->aux_stream : st;
        if (overlap) HIPCHK(hipStreamWaitEvent(fs, s->ev_fork, 0));
        {
            ProfScope ps(s, CLS_ST_FACTOR, fs);
            if (s->stable_factor >= 1) {
                // row-wise, from U alone (the scratch entry it would read IS fl(U * w): see k_st_factor_rows)
                const unsigned gy = (unsigned)((n + FROW_H - 1) / FROW_H);
                if (n >= 8192)
                    hipLaunchKernelGGL((k_st_factor_rows<2048, 2>), dim3(gy, (unsigned)((n + 2047) / 2048)), dim3(256), 0,
                                       fs, s->d_Q, ld, n, beta2, (const double*)w, s->d_st);
                else
                    hipLaunchKernelGGL((k_st_factor_rows<512, 4>), dim3(gy, (unsigned)((n + 511) / 512)), dim3(256), 0,
                                       fs, s->d_Q, ld, n, beta2, (const double*)w, s->d_st);
            } else {
                const unsigned nt64 = (unsigned)((n + 63) / 64);  // 64x64 tiles, scratch triangle transposed through LDS
                hipLaunchKernelGGL(k_st_factor, dim3(nt64, nt64), dim3(256), 0, fs, s->d_Q, ld, n, beta2, s->d_st);
            }
            HIPCHK(hipGetLastError());
        }
        if (overlap) {
            HIPCHK(hipEventRecord(s->ev_join, fs));
            HIPCHK(hipStreamWaitEvent(st, s->ev_join, 0));
        }
    }
    return 0;
}

}  // namespace
