// ell_resident_capi.inc.hpp -- queue runs with the matrix parked on-chip: can this handle run resident (resident_setup,
// resident_ok) and one batch as one cooperative launch (resident_run), abandoned and undone as a whole when a wait gives up.
// Needs: ell_primitives_capi.inc.hpp, ellstable_capi.inc.hpp (CoresScope).  DESIGN.md section 3.5; resident_kernels.hpp.

namespace {

// ---- queue runs with the matrix parked on-chip (resident_kernels.hpp) ------------------------------------------------
// Chosen for a run of at least RS_MIN_COUNT queued cuts of an unsharded Ell handle whose lower triangle fits the
// register files: R = the smallest super-tile edge with no more super-tiles than the device has CUs, and one workgroup
// of k_ell_resident<R> must fit a CU.  Not while no_defer_trick is set (the kernel has no scale pass) or before a
// non-symmetric input has been mirrored, and not for the device-resident cutting-plane loops (tolerance stop).
constexpr long long RS_MIN_COUNT = 4;

int resident_setup(ellhip_space* s) {  // once per handle: can this n run resident on this device, and with which R?
    if (s->rs_R != 0) return 0;
    if (s->variant != ELLHIP_SPACE_ELL || s->sharded) {
        s->rs_R = -1;
        return 0;
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, s->device));  // (rs_R stays 0 on every failure: the next queue run asks again)
    const int T = (int)((s->n + RS_TS - 1) / RS_TS);
    for (int r = 1; r <= RS_RMAX; ++r) {
        const int S = (T + r - 1) / r;
        if (S > RS_SMAX || S * (S + 1) / 2 > prop.multiProcessorCount) continue;
        int occ = 0;
        const void* k = r == 1 ? (const void*)k_ell_resident<1> : (r == 2 ? (const void*)k_ell_resident<2> : (const void*)k_ell_resident<3>);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, RS_THREADS, 0) != hipSuccess || occ < 1) continue;
        const size_t G = (size_t)S * (S + 1) / 2, NV = 2 * (size_t)r * RS_TS;
        const size_t mark = s->mem.mark();
        hipError_t e = s->mem.device(s->d_rs_part, 2 * G * NV * sizeof(double));
        if (e == hipSuccess) e = s->mem.device(s->d_rs_omega, 2 * G * sizeof(double));
        if (e == hipSuccess) e = s->mem.device(s->d_rs_bar, RS_BAR_WORDS * sizeof(unsigned));
        if (e == hipSuccess) e = s->mem.device(s->d_rs_xc0, (size_t)s->n * sizeof(double));
        if (e == hipSuccess) e = s->mem.device(s->d_rs_st0, sizeof(DevState));
        if (e != hipSuccess) {
            s->mem.rollback(mark);
            return fail(ELLHIP_E_HIP, "buffers of the resident queue runs", e);
        }
        s->rs_R = r;
        s->rs_S = S;
        return 0;
    }
    s->rs_R = -1;  // does not fit this device
    return 0;
}

bool resident_ok(ellhip_space* s, long long count) {
    if (!s->resident || count < RS_MIN_COUNT || s->variant != ELLHIP_SPACE_ELL || s->sharded || s->no_defer_trick || s->needs_mirror)
        return false;
    if (s->h_result && s->h_result->tol >= 0.0) return false;
    if (resident_setup(s) != 0) return false;
    return s->rs_R > 0;
}

// (one resident grid per device at a time within this process, and none beside an EllStable persistent solve: CoresScope)
constexpr int RS_FALLBACK = 1;  // resident_run: the batch did not run (or was abandoned and undone): take the streamed schedule

// One batch = one cooperative launch.  The call returns when the batch has finished (one stream synchronisation per
// batch: the verdict "committed or abandoned" is needed before anything else may be enqueued behind it).
//   0            the batch ran: Q (lower triangle), xc, DevState and the queue results are those of `count` more cuts;
//   RS_FALLBACK  nothing happened as far as the caller can tell -- the launch was refused (the grid cannot be co-resident
//                on this device as it is partitioned now) or a bounded wait inside the kernel gave up, in which case no
//                tile was written back (rs_commit) and xc / DevState / the batch's queue results have been restored from
//                the snapshots taken below.  The caller continues with the streamed schedule; so does the handle from
//                now on (s->resident = 0).
int resident_run(ellhip_space* s, long long first, long long count) {
    // the lower triangle must be current: commit a pending shrink, apply what the recorded schedule holds; a primed
    // gradient is simply dropped (the kernel forms every Q g itself)
    int rc = ensure_committed(s);
    if (rc) return rc;
    if (s->npend > 0) {
        rc = flush_pending(s, nullptr, nullptr);
        if (rc) return rc;
    }
    drop_prime(s);
    s->xc_host_valid = false;
    ResidentArgs A{};
    A.Q = s->d_Q;
    A.ld = s->ld;
    A.n = s->n;
    A.T = (int)((s->n + RS_TS - 1) / RS_TS);
    A.R = s->rs_R;
    A.S = s->rs_S;
    A.qgrads = s->d_qgrads;
    A.qparams = s->d_qparams;
    A.qstatus = s->d_qstatus;
    A.qtsq = s->d_qtsq;
    A.first = first;
    A.count = count;
    A.xc = s->d_xc;
    A.st = s->d_st;
    A.part = s->d_rs_part;
    A.omega_part = s->d_rs_omega;
    A.ctr = s->d_rs_bar;
    A.stamps = nullptr;
    A.calc = EllCalcDev::make(s->n, s->use_parallel_cut);
    A.fault_at = s->rs_fault_at;
    const unsigned G = (unsigned)(s->rs_S * (s->rs_S + 1) / 2);
    CoresScope alone(s);  // (held until the batch has finished: the function synchronises the stream before it returns)
    hipLaunchKernelGGL(k_rs_prepare, dim3((unsigned)std::max<long long>(1, std::min<long long>(32, s->n / 256))), dim3(256), 0, s->stream,
                       (const double*)s->d_xc, s->d_rs_xc0, s->n, (const DevState*)s->d_st, s->d_rs_st0, s->d_rs_bar);
    HIPCHK(hipGetLastError());
    {
        ProfScope ps(s, CLS_RESIDENT);
        const void* k = s->rs_R == 1 ? (const void*)k_ell_resident<1> : (s->rs_R == 2 ? (const void*)k_ell_resident<2> : (const void*)k_ell_resident<3>);
        void* args[] = {&A};
        // ELLHIP_OPT_RESIDENT = 1 (default): a cooperative launch -- the runtime refuses a grid that cannot be co-resident and
        // runs one cooperative grid at a time, across processes too; measured at the plain launch's speed (n = 4096, 200 cuts
        // per batch: 1.84 vs 1.87 ms).  2: a plain launch, for a stack without cooperative launches.  Either way the batches
        // of this process are serialised per device by CoresScope (held here until the batch has finished),
        // and whatever still keeps workgroups out ends in the bounded waits giving up: the batch is abandoned as a whole
        // and rerun on the streamed schedule (below).
        const hipError_t e = s->resident == 1 ? hipLaunchCooperativeKernel(k, dim3(G), dim3(RS_THREADS), args, 0, s->stream)
                                              : hipLaunchKernel(k, dim3(G), dim3(RS_THREADS), args, 0, s->stream);
        if (e != hipSuccess) {
            // not co-resident on this device (partitioned, CU mask, ...): no resident batches on this handle any more
            (void)hipGetLastError();
            s->resident = 0;
            return RS_FALLBACK;
        }
    }
    HIPCHK(hipMemcpyAsync(s->h_result, s->d_st, sizeof(DevState), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->h_result->solve_err) {
        // abandoned: Q was not written.  Put back what the kernel's cuts wrote on the way -- xc (the diagonal workgroups),
        // the scalar state, the batch's queue results ("not run yet") -- and let the streamed schedule take the batch.
        HIPCHK(hipMemcpyAsync(s->d_xc, s->d_rs_xc0, (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        HIPCHK(hipMemcpyAsync(s->d_st, s->d_rs_st0, sizeof(DevState), hipMemcpyDeviceToDevice, s->stream));
        HIPCHK(hipMemsetAsync(s->d_qstatus + first, 0xff, (size_t)count * sizeof(int), s->stream));
        HIPCHK(hipMemsetAsync(s->d_qtsq + first, 0, (size_t)count * sizeof(double), s->stream));
        HIPCHK(hipMemcpyAsync(s->h_result, s->d_st, sizeof(DevState), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        s->resident = 0;
        s->rs_abandoned += 1;
        (void)fail(0, "a resident batch was abandoned (bounded in-launch wait) and rerun on the streamed schedule; "
                      "ELLHIP_OPT_RESIDENT is now 0 on this handle");
        return RS_FALLBACK;
    }
    // The kernel wrote the lower triangle (diagonal tiles whole).  Where the streamed schedule of this handle reads
    // full rows, the mirrored half is rebuilt at once; a handle on the lower-triangle schedule leaves it stale as its
    // own apply passes do (make_q_current mirrors before anything observes Q).
    if (symv_ok(s) && s->apply_lower) {
        s->upper_stale = true;
    } else {
        const unsigned t = (unsigned)((s->n + 31) / 32);
        hipLaunchKernelGGL(k_mirror_lower_now, dim3(t, t), dim3(256), 0, s->stream, s->d_Q, s->ld, s->n);
        HIPCHK(hipGetLastError());
        s->upper_stale = false;
    }
    s->shrink_pending = false;
    s->kappa = s->h_result->kappa;
    s->tsq = s->h_result->tsq;
    s->scalars_stale = false;
    return 0;
}

}  // namespace
