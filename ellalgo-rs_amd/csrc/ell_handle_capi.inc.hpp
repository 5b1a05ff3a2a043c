// ell_handle_capi.inc.hpp -- what every piece of the Ell / EllStable engine's host side starts from: the error record (fail,
// HIPCHK), fill_now, the per-handle options and the process-wide defaults, the handle itself (ellhip_space: its options, the
// record a clone inherits, the buffers and the pipeline state), DeviceGuard and the per-kernel-class event timing.
// Needs: include/ellhip.h, the kernel headers (SYMV_SEG, DevState, StPend, LiveMirror, ...) and device_allocs.hpp.
// First of the engine's pieces in ellhip_capi.hip.  DESIGN.md section 2 (buffers), 13 (options).

namespace {

thread_local std::string g_last_error = "";

int fail(int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    else
        snprintf(buf, sizeof buf, "%s", what);
    g_last_error = buf;
    return code;
}

#define HIPCHK(expr)                                                \
    do {                                                            \
        hipError_t _e = (expr);                                     \
        if (_e != hipSuccess) return fail(ELLHIP_E_HIP, #expr, _e); \
    } while (0)

// hipMemset on device memory is enqueued on the null stream and may return before the fill has run, and every handle's stream is
// non-blocking: a kernel launched right afterwards on the handle's stream can run BEFORE the fill and be overwritten by it (seen once in
// 3600 state-machine walks: the first queued cut's tsq read back as 0 -- the fill of ellhip_queue_upload had landed behind the cut).
// Fills are therefore waited for: the same null-stream hipMemset as before, then a wait for the null stream.  (Moving the fills to the
// handle's own stream changed what the host threads of the multi-rank tests wait for and two suite runs in a row lost a rank case;
// this form changes nothing but the missing wait.)
hipError_t fill_now(void* p, int value, size_t bytes, hipStream_t /*the handle's stream: documentation only*/) {
    const hipError_t e = hipMemset(p, value, bytes);
    return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
}

struct ProfEvent {
    hipEvent_t a, b;
    int cls;
};

// The per-handle options (ellhip_set_option / ellhip_get_option) with their factory values: the measured best on MI355X;
// nothing here is read from the environment.  Every handle carries one (ellhip_space derives from it), g_defaults holds
// what a NEW handle starts with.  A new option is a field here and a row in g_option_table, nothing else.
struct SpaceOptions {
    long long symv = 1;              // ELLHIP_OPT_SYMV: allow the lower-triangle GEMV in deferred mode
    long long symv_min_n = 5120;     // ELLHIP_OPT_SYMV_MIN_N: below this the full-row pass wins for synchronous updates (tools/midsize_sweep.py)
    long long apply_lower = 1;       // ELLHIP_OPT_APPLY_LOWER: with symv: apply passes touch the lower triangle only
    long long apply_kernel = -1;     // ELLHIP_OPT_APPLY_KERNEL: lower-triangle apply pass: 2 = k_apply_mfma, 1 = k_apply_lower, 0 = k_sweep_apply<LOWER> (depth 8); -1 = 2 at depth 24, else 1
    long long fuse_dots = 1;         // ELLHIP_OPT_FUSE_DOTS: unsharded lower-triangle schedule: k_symv_reduce also yields the scalar stage's dot products
    long long resident = 1;          // ELLHIP_OPT_RESIDENT: queue runs with the matrix parked on-chip (resident_kernels.hpp)
    long long overlap = 1;           // ELLHIP_OPT_OVERLAP: the next cut's GEMV / the next group's products on a second stream
    long long lookahead = 32;        // ELLHIP_OPT_LOOKAHEAD: GEMVs of up to this many consecutive queued cuts in ONE pass over Q_base
    long long queue_depth = 48;      // ELLHIP_OPT_QUEUE_DEPTH: recorded updates a queue run on the group stage lets pile up before an apply pass (0: the handle's depth)
    long long apply_symm = 1;        // ELLHIP_OPT_APPLY_SYMM: that apply pass rides on the next group's product pass (k_apply_symm_q; queue_run_multi)
    long long packed_operands = 1;   // ELLHIP_OPT_PACKED_OPERANDS: the matrix-core passes fetch gradients and recorded vectors, and store column sums,
                                     // 16 bytes per lane (k_pack_operands: gP in d_gT, colpart2 in d_colpart_m; unsharded handles)
    long long stable_solve = 3;      // ELLHIP_OPT_STABLE_SOLVE: 0: one launch per block; 1: persistent solves; 2: persistent + helper workgroups; 3: 2 on the mirrored layout
    long long stable_factor = 2;     // ELLHIP_OPT_STABLE_FACTOR: 0: tile kernel that reads the scratch triangle; 1: row kernel from U alone, beside the
                                     // backward solve; 2: factor tiles pulled inside the helped backward solve's launch
};
// ... plus the values that exist as defaults only (ellhip_set_default_option; process-wide, not thread-safe by contract)
struct Defaults : SpaceOptions {
    long long auto_defer = 1;        // ELLHIP_OPT_AUTO_DEFER
    long long pad = -1;              // ELLHIP_OPT_PAD: extra doubles per row of Q; -1 = by size (create_impl)
    long long lp_grid = 0;           // ELLHIP_OPT_LP_GRID: workgroups per LowpassOracle scan launch; 0 = by size
    long long lp_wide = -1;          // ELLHIP_OPT_LP_WIDE: column-split scan kernel; -1 = by size
    long long batch_threads = 0;     // ELLHIP_OPT_BATCH_THREADS: threads per workgroup of the batched engine; 0 = by size
    long long stage_direct = 1;      // ELLHIP_OPT_STAGE_DIRECT: on large-BAR systems the host writes gradients straight into device memory
};
Defaults g_defaults;

struct Shape {
    int rw = 0, unr = 0, nt = 0;
};

// What a clone inherits besides the options and the device's own state, as one record (ellhip_space derives from it;
// create_impl, pick_shape and the setters fill it, ellhip_clone copies it in one assignment).  A new configuration field
// goes here, or the clone loses it.  Not here: kappa / tsq (read from the device state), defer (through
// ellhip_set_defer_depth, which also allocates), rs_fault_at (a test hook stays with its handle).
struct SpaceInherited {
    int variant = ELLHIP_SPACE_ELL;
    long long n = 0, ld = 0, row0 = 0, nrows = 0;
    int device = 0;
    bool sharded = false;
    int no_defer_trick = 0;
    int use_parallel_cut = 1;
    bool needs_mirror = false;       // caller-supplied non-symmetric matrix, no successful update yet
    Shape sh_gemv, sh_rank1, sh_fused, sh_apply;  // launch shapes per role: chosen by size (pick_shape), nothing sets them afterwards
    int symv_rw = 2;                 // rows in flight per thread of the lower-triangle GEMV (symv_alloc)
    int symv_seg = SYMV_SEG;         // segment width of the lower-triangle GEMV's tiles (see symv_alloc)
    bool shard_symmetric = false;    // row shard whose GEMVs are partial symmetric sums (ellhip_set_shard_symmetric)
    bool upper_stale = false;        // strict upper triangle of Q is out of date (see flush_pending)
};

}  // namespace

struct ellhip_space : SpaceOptions, SpaceInherited {
    Allocs mem;                      // owner of every d_* / h_* buffer below that is not an alias (device_allocs.hpp)

    double* d_Q = nullptr;           // nrows * ld
    double* d_xc = nullptr;          // n
    double* d_stage[2] = {nullptr, nullptr};   // gradient of slot 0 / 1 (n doubles)
    bool stage_direct = false;       // d_stage is fine-grained device memory the HOST writes through the PCIe BAR (large-BAR systems)
    double* d_gt_own[2] = {nullptr, nullptr};  // Q*g of slot 0 / 1 (n doubles)
    double* d_gt[2] = {nullptr, nullptr};      // buffers in use (own or caller's)
    double* d_work = nullptr;        // EllStable vectors: w, z, gg, q, beta2
    double* d_hpart = nullptr;       // EllStable forward solve with helper workgroups: the helpers' hand-over buffer (n)
    int* d_fnext = nullptr;          // queue position of the factor tiles (reset by k_st_post before every launch)
    int* d_ftiles16 = nullptr;       // k_st_bwd_factor_helped: 16-row tiles (row group << 4 | segment)
    int nftiles16 = 0;
    double* d_qhpart = nullptr;      // ... and the backward helpers' hand-over buffer (n)
    int persist_cap_h = 0;           // resident-workgroup limit of the helped solves (CU count x occupancy of k_st_fwd_helped)
    // EllStable, ELLHIP_OPT_STABLE_SOLVE = 3: the mirrored layout (ellstable_kernels.hpp, StPend)
    bool st_mirrored = false;        // host view: the handle's solves run on the mirrored layout (the device's own flag, StPend.mirrored,
                                     // says whether the lower triangle really holds the mirrored factor: not after a halted queue)
    StPend* d_stpend = nullptr;
    double* d_rbuf = nullptr;        // [2][n] running row scales of the factor (two buffers: StPend says who reads which)
    double* d_wkeep = nullptr;       // [n] w of the last forward solve that really ran (what the scratch triangle is made of)
    int st_since_enter = 0;          // updates issued since the layout was entered (re-entered every ST_MIRROR_PERIOD)
    bool st_prev_persist = true;     // the previous update ran the persistent / helped solves: its k_st_post re-armed their
    bool st_prev_helped = true;      // hand-over buffers for this one (true at creation: alloc_common arms them all)
    double* d_partial = nullptr;     // per-workgroup partial sums of omega (64)
    double* d_pend = nullptr;        // deferred mode: MAXPEND pending gt vectors (n each)
    double* d_cpend = nullptr;       // deferred mode: their coefficients sigma/omega
    double* d_rowpart = nullptr;     // symmetric GEMV: per-segment row partial sums  [n/SYMV_SEG][n]
    double* d_colpart = nullptr;     // symmetric GEMV: per-strip column partial sums [n/SYMV_H][n]
    // pipelined queue runs on the lower-triangle schedule (ELLHIP_OPT_OVERLAP): the next cut's GEMV is issued on a second
    // stream beside this cut's reduction + scalar stage, into the other of two sets of partial sums
    double* d_rowpart2 = nullptr;
    double* d_colpart2 = nullptr;
    int part_set = 0;                // the set the primed gradient's GEMV wrote / writes (see rowpart_of)
    hipStream_t symv_stream = nullptr;
    // ... and with the GEMVs of up to `lookahead` consecutive queued cuts computed in ONE pass over Q_base (k_symv_multi,
    // ELLHIP_OPT_LOOKAHEAD): vector l of a group writes partial-sum set 2 + l (slices of one allocation)
    double* d_rowpart_m = nullptr;   // [MULTI_MAX][nsegs][n]
    double* d_colpart_m = nullptr;   // [MULTI_MAX][nstrips][n]
    double* d_gT = nullptr;          // [n][16]: a group's gradients side by side (operand layout of k_symm_mfma)
    double* d_pendP = nullptr;       // [n / 16][KS / 2][64][2]: the recorded vectors in the fused pass' operand order (MAXPEND n doubles)
    SymmTile* d_symm_tiles = nullptr;  // k_symm_mfma_q's tiles, largest first
    unsigned* d_symm_queue = nullptr;  // its two counters (one per half of the partial-sum sets), 128 bytes apart
    int symm_ntiles = 0, symm_wgs = 0;
    // ... and the group's scalar stage (group_kernels.hpp)
    double* d_grpY = nullptr;        // [GRP_MAX][n]: y_l = Q_base g_l of the group's cuts
    double* d_gpart = nullptr;       // [GRP_MAX][ceil(n/128)][MAXPEND + 1]
    double* d_cpart = nullptr;       // [ceil(n/128)][GRP_MAX * GRP_MAX]
    double* d_gsums = nullptr;       // [GRP_MAX][MAXPEND + 1] + [GRP_MAX][GRP_MAX]: their sums over the blocks
    GroupOut* d_gout = nullptr;
    // a symmetric row shard's group runs: the owner's all-reduce of the group's partial products (count doubles at buf, in
    // place, on `stream`); set by sharded_capi.inc.hpp around its call of queue_run_multi
    int (*grp_exchange)(void* ctx, double* buf, long long count, hipStream_t stream) = nullptr;
    void* grp_exchange_ctx = nullptr;
    hipEvent_t ev_symv = nullptr;    // side_mark: what was issued on the second stream has finished
    hipEvent_t ev_side_go = nullptr; // side_fork: everything enqueued on the handle's stream up to the fork
    bool side_busy = false;          // work issued on the second stream has not been joined yet (side_fork .. side_join)
    // queue runs with the matrix parked on-chip (resident_kernels.hpp, ELLHIP_OPT_RESIDENT)
    int rs_R = 0, rs_S = 0;          // super-tile edge / rows chosen for this n and device (0: does not fit)
    double* d_rs_part = nullptr;     // [2][grid][2 R 64]
    double* d_rs_omega = nullptr;    // [2][grid]
    unsigned* d_rs_bar = nullptr;    // RS_BAR_WORDS
    double* d_rs_xc0 = nullptr;      // xc at the start of the batch in flight (restored when the batch is abandoned)
    DevState* d_rs_st0 = nullptr;    // ... and the scalar state
    long long rs_fault_at = -1;      // ELLHIP_OPT_RESIDENT_FAULT (test hook; deliberately outside SpaceOptions: a clone does not inherit it)
    long long rs_abandoned = 0;      // batches abandoned and rerun on the streamed schedule (ELLHIP_OPT_RESIDENT_ABANDONED)
    int dots_np = 0;                 // > 0: d_partial holds dot products of the primed gradient for this depth: [ceil(n/128)][dots_np + 1]
                                     // from k_symv_reduce, or [scalar_groups(n)][...] WITHOUT the g.y column from k_sweep_gemv_dots
    bool dots_need_gy = false;       // the latter: k_scalar_apply_def forms g.y itself
    int defer = 1;                   // 1 = shrink Q at every cut; MAXPEND = record and apply in batches
    int npend = 0;                   // updates recorded since the last flush (host view, optimistic in queue mode)
    int* d_flags = nullptr;          // EllStable persistent solves: block-ready flags (forward | backward)
    int epoch = 0;                   // hand-off epoch, bumped per persistent launch
    int persist_cap1 = 0;            // workgroups of the persistent solves the device holds at once (CU count x occupancy)
    DevState* d_st = nullptr;

    double* h_stage[2] = {nullptr, nullptr};  // pinned, n doubles each
    DevState* h_result = nullptr;             // pinned
    // live updates (ellhip_update / ellhip_cut): k_publish writes the scalar state and the centre into these right behind
    // the scalar stage and the host polls the sequence number -- no device-to-host copy, no wait for the whole stream
    LiveMirror* h_live = nullptr;             // pinned, fine-grained
    double* h_xc = nullptr;                   // pinned, fine-grained: the centre as of the last published update
    unsigned long long live_seq = 0;
    unsigned* d_pub_arrived = nullptr;        // k_publish: workgroups that have pushed their slice of the centre
    bool xc_host_valid = false;               // h_xc equals d_xc (nothing has written the centre on the device since)
    bool live_arm = false;                    // the do_cut in progress belongs to a live update: the scalar stage may publish itself
    bool live_done = false;                   // ... and did (live_publish has nothing left to launch)

    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;           // EllStable: factor update runs beside the persistent backward solve
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;

    // pipeline state
    int cur = 0;                  // slot of the primed / current gradient
    bool primed = false;          // gt[cur] = Q * g[cur] is valid (or in flight)
    const double* g_cur = nullptr;  // device pointer of the primed gradient (stage slot or queue entry)
    bool shrink_pending = false;  // a cut succeeded (or may have: queue mode) and Q has not been shrunk yet
    bool in_two_phase = false;    // update_begin issued, update_end not yet
    CutParams two_phase_cp{};     // cut scalars kept between begin and end
    int dir = 0;                  // direction of the next pass over Q (serpentine)
    long long primed_qindex = -1; // queue index the primed gradient belongs to (-1: a direct gradient)

    // cached scalars (refreshed by every synchronous read-back; `scalars_stale`: queue cuts have been issued since)
    double kappa = 1.0, tsq = 0.0;
    bool scalars_stale = false;

    // device-resident cut queue
    long long qk = 0;
    CutParams* d_qparams = nullptr;
    double* d_qgrads = nullptr;
    int* d_qstatus = nullptr;
    double* d_qtsq = nullptr;

    // per-kernel event timing
    bool profile = false;
    std::vector<ProfEvent> prof_events;
    size_t prof_used = 0;
    double prof_ms[ELLHIP_NKERNEL_CLASSES] = {0};
    long long prof_cnt[ELLHIP_NKERNEL_CLASSES] = {0};
};

namespace {

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// ---- profiling helpers ---------------------------------------------------------------------
enum : int { CLS_GEMV = 0, CLS_SCALAR = 1, CLS_RANK1 = 2, CLS_ST_FWD = 3, CLS_ST_BWD = 4, CLS_ST_FACTOR = 5, CLS_FUSED = 6, CLS_APPLY = 7, CLS_APPLY_GEMV = 8, CLS_SYMV = 9, CLS_SYMV_REDUCE = 10, CLS_LP_SCAN = 11, CLS_LP_FINAL = 12, CLS_RESIDENT = 13 };

int prof_flush(ellhip_space* s) {
    for (size_t i = 0; i < s->prof_used; ++i) {
        ProfEvent& pe = s->prof_events[i];
        HIPCHK(hipEventSynchronize(pe.b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, pe.a, pe.b));
        s->prof_ms[pe.cls] += ms;
        s->prof_cnt[pe.cls] += 1;
    }
    s->prof_used = 0;
    return 0;
}

struct ProfScope {
    ellhip_space* s;
    ProfEvent* pe = nullptr;
    hipStream_t stream;
    ProfScope(ellhip_space* sp, int cls, hipStream_t on = nullptr) : s(sp), stream(on ? on : sp->stream) {
        if (!s->profile) return;
        if (s->prof_used == s->prof_events.size()) {
            if (s->prof_events.size() >= 8192) {
                if (prof_flush(s) != 0) return;
            } else {
                ProfEvent e;
                if (hipEventCreate(&e.a) != hipSuccess) return;
                if (hipEventCreate(&e.b) != hipSuccess) {
                    (void)hipEventDestroy(e.a);
                    return;
                }
                e.cls = cls;
                s->prof_events.push_back(e);
            }
        }
        pe = &s->prof_events[s->prof_used++];
        pe->cls = cls;
        (void)hipEventRecord(pe->a, stream);
    }
    ~ProfScope() {
        if (pe) (void)hipEventRecord(pe->b, stream);
    }
};

}  // namespace
