// ell_group_capi.inc.hpp -- queue runs that form the products of a group of cuts in one pass over the lower triangle
// (queue_run_multi): the matrix-core product pass and the fused apply-and-product pass (ONE launcher, group_pass_launch, for
// the runs and for the empty launches that warm every form a handle can take), the group's buffers (multi_setup / multi_fill
// / multi_free), one half of them as a value (GroupHalf), and the group's scalar stage.
// Needs: ell_queue_capi.inc.hpp, launch_dispatch.hpp.  DESIGN.md section 3.6; group_kernels.hpp for the stage.

namespace {

// ---- pipelined queue runs with several cuts' GEMVs in one pass over Q_base (ELLHIP_OPT_LOOKAHEAD) ---------------------
// The same observation taken further: between two apply passes EVERY queued cut's y = Q_base g refers to the same
// matrix, so the products of a group of L consecutive queued cuts are formed in ONE pass over the lower triangle
// (k_symv_multi: each element loaded once, used for L gradients) -- (4 / L) n^2 bytes per update instead of 4 n^2.
// The reductions and scalar stages then run cut by cut as before (cut l's correction needs the vector cut l - 1
// recorded).  A group never reaches across an apply pass or the end of the run; a cut that arrives primed (by an
// earlier call) is taken by itself first.  Two kernels:
//   lookahead <= 3   k_symv_multi on the vector ALU: per vector k_symv's arithmetic, bit-identical results;
//   lookahead >  3   k_symm_mfma on the FP64 matrix cores (n a multiple of 64): up to 16 gradients in the time of ONE
//                    pass; y differs from k_symv's by a few ulp (own association, fused multiply-add) -- inside the
//                    contract's 1e-10, not bit-identical to the other schedules.
bool multi_ok(const ellhip_space* s) {
    return s->lookahead > 1 && s->variant == ELLHIP_SPACE_ELL && !s->sharded && symv_ok(s);
}
bool multi_mfma(const ellhip_space* s) { return s->lookahead > MULTI_VALU_MAX && (s->n % 64) == 0; }
// a symmetric row shard: the matrix-core groups only, and every cut through them (a single cut's GEMV would need the
// owner's per-cut collective in between); its owner calls queue_run_multi with grp_exchange set
bool multi_shard_ok(const ellhip_space* s) {
    return s->variant == ELLHIP_SPACE_ELL && s->sharded && s->shard_symmetric && symv_ok(s) && multi_mfma(s) &&
           (s->row0 % 64) == 0 && ((s->row0 + s->nrows) % 64 == 0 || s->row0 + s->nrows == s->n);
}

constexpr int MULTI_NO_MEMORY = 1;  // multi_setup: the buffers do not fit; the handle has been switched to lookahead 1

// ELLHIP_OPT_PACKED_OPERANDS: the passes of this handle's group runs take the packed forms (a queue run keeps one form from its
// first pass to its last stage: the option is read here only, and set between runs).  Row shards stay on the unpacked kernels.
bool packed_on(const ellhip_space* s) { return s->packed_operands != 0 && !s->sharded && s->symm_ntiles > 0 && s->d_pendP != nullptr; }

// Which form of k_group_reduce_p reads the column sums of a group of g cuts (group_kernels.hpp).  The pass has just written them:
// the lower triangle of (g + 1) / 2 planes of 16 bytes per strip and column.  Up to about the 256 MiB of the Infinity Cache most of
// them are still on the die and plain loads find them there (n = 16384: a group of 16 is 256 MiB, and non-temporal loads cost it
// 15 us of 60); well beyond, they come from HBM and are read once: the streaming form (a group of 32: 129 us instead of 175).
// Same bits either way.
bool group_reduce_streams(const ellhip_space* s, int g) {
    const double bytes = (double)((g + 1) / 2) * (double)colpart_elems(s) * 16.0 / 2.0;
    return bytes > 1.5 * 256.0 * 1024.0 * 1024.0;
}

// Half `h` of the group runs' buffers: the next group's products are formed in one half while this group's stage reads the other.
struct GroupHalf {
    double* gT;       // the group's gradients in the pass' operand order
    double* rowp;     // MULTI_MAX sets of row partial sums ...
    double* colp;     // ... and of column partial sums
    unsigned* queue;  // the tile counter of the passes on this half
    static int nvw(int lv) { return lv > SMM_NV ? SMM_NV2 : SMM_NV; }  // gradients the pass is as wide as: one or two 16-wide column tiles
};
GroupHalf group_half(const ellhip_space* s, int h) {
    return {s->d_gT + (size_t)h * (size_t)s->n * MULTI_MAX, s->d_rowpart_m + (size_t)h * MULTI_MAX * rowpart_elems(s),
            s->d_colpart_m + (size_t)h * MULTI_MAX * colpart_elems(s), s->d_symm_queue + 32 * h};
}

// The operands of a product pass: the gradients in the pass' order in half `half` of gT, and that half's tile counter rewound.  It
// writes nothing else, and the last reader of both is the pass that ran on that half before.
void symm_pack_go(ellhip_space* s, const double* g_dev, int lv, hipStream_t st, int half) {
    const GroupHalf H = group_half(s, half);
    const int nvw = GroupHalf::nvw(lv);
    if (packed_on(s))
        hipLaunchKernelGGL(k_pack_operands, dim3((unsigned)(s->n * (nvw / SMM_NV) / 32)), dim3(256), 0, st, g_dev, s->n, lv, s->n, H.gT, H.queue,
                           nvw / SMM_NV, (const double*)nullptr, (double*)nullptr, 0);
    else
        hipLaunchKernelGGL(k_pack_grads, dim3((unsigned)((s->n * nvw + 255) / 256)), dim3(256), 0, st, g_dev, s->n, lv, s->n, H.gT, H.queue, nvw);
}

// One form of a matrix-core pass of the group runs.  np = 0: the product pass (k_symm_mfma_q, two column tiles: k_symm_mfma_q2);
// np = MAXPEND or 24: the apply pass of that rank fused with it (k_apply_symm_q).  NT and the segment width follow the handle.
struct GroupPassForm {
    int np;
    bool two, packed;
};
// THE launcher of those passes: the argument list of each of the two families once, every form a template argument.  The queue
// runs call it with their grid, group and tile count; multi_fill with one workgroup and no tiles.
void group_pass_launch(ellhip_space* s, GroupPassForm f, const GroupHalf& H, int lv, hipStream_t st, unsigned wgs, int ntiles) {
    const long long relems = (long long)rowpart_elems(s), celems = (long long)colpart_elems(s);
    with_bool(s->sh_gemv.nt != 0, [&](auto ntc) {
        with_bool(s->symv_seg == SYMV_SEG, [&](auto wide) {
            with_bool(f.two, [&](auto two) {
                with_bool(f.packed, [&](auto pk) {
                    constexpr bool NT = decltype(ntc)::value, TWO = decltype(two)::value, PK = decltype(pk)::value;
                    constexpr int SEG = decltype(wide)::value ? SYMV_SEG : SYMV_SEG_SMALL;
                    auto product = [&](auto kernel) {
                        hipLaunchKernelGGL(kernel, dim3(wgs), dim3(256), 0, st, (const double*)s->d_Q, s->ld, s->n, s->row0,
                                           (const double*)H.gT, lv, H.rowp, H.colp, relems, celems, (const DevState*)s->d_st,
                                           (const SymmTile*)s->d_symm_tiles, ntiles, H.queue);
                    };
                    if (f.np == 0) {
                        if constexpr (TWO) product(k_symm_mfma_q2<NT, SEG, PK>);
                        else product(k_symm_mfma_q<NT, SEG, PK>);
                        return;
                    }
                    with_int(Ints<MAXPEND, 24>{}, f.np, [&](auto npc) {
                        hipLaunchKernelGGL((k_apply_symm_q<decltype(npc)::value, NT, SEG, TWO, PK>), dim3(wgs), dim3(256), 0, st, s->d_Q,
                                           s->ld, s->n, (const double*)s->d_pend, (const double*)s->d_cpend, (const double*)H.gT, lv,
                                           H.rowp, H.colp, relems, celems, (const DevState*)s->d_st, (const SymmTile*)s->d_symm_tiles,
                                           ntiles, H.queue, (const double*)s->d_pendP);
                    });
                });
            });
        });
    });
}
// Every form the group runs of this handle can take, in the order multi_fill warms them: both widths of the product pass,
// unpacked, and packed unless the handle is a shard; the fused pass (unsharded, row0 = 0) at both ranks and widths, unpacked
// and packed.  Returns how many.
int group_pass_forms(const ellhip_space* s, GroupPassForm out[12]) {
    int k = 0;
    for (int pk = 0; pk <= (s->sharded ? 0 : 1); ++pk)
        for (int two = 0; two <= 1; ++two) out[k++] = {0, two != 0, pk != 0};
    if (s->row0 == 0 && !s->sharded)
        for (int pk = 0; pk <= 1; ++pk)
            for (int np : {(int)MAXPEND, 24})
                for (int two = 1; two >= 0; --two) out[k++] = {np, two != 0, pk != 0};
    return k;
}

// ELLHIP_OPT_APPLY_SYMM: the rank of the apply pass flush_pending would run on the matrix cores right now (k_apply_mfma<48> when
// more are recorded than the depth, <24> at depth 24 where the option picks that kernel), 0 where it would pick another kernel or
// the fused pass does not exist (shards: row0 != 0; the tile queue needs n % 64 == 0)
int apply_symm_np(const ellhip_space* s) {
    if (!s->apply_symm || s->sharded || s->variant != ELLHIP_SPACE_ELL || !s->apply_lower || !symv_ok(s) || !multi_mfma(s) ||
        s->symm_ntiles == 0)
        return 0;
    if (s->npend > s->defer) return MAXPEND;
    const int apply_kernel = s->apply_kernel < 0 ? (s->defer == 24 ? 2 : 1) : s->apply_kernel;
    return (apply_kernel == 2 && s->defer == 24) ? 24 : 0;
}

// The apply pass a full set of recorded updates still owes, fused with the product pass of the group at `g_dev` (k_apply_symm_q:
// one sweep over the lower triangle instead of k_apply_mfma's and k_symm_mfma_q's), then the slots are forgotten as after
// flush_pending.  `owed` is cleared once the pass is issued.
int apply_symm_go(ellhip_space* s, const double* g_dev, int lv, int half, int np, bool& owed) {
    {
        ProfScope ps(s, CLS_APPLY_GEMV);
        const GroupHalf H = group_half(s, half);
        const int nvw = GroupHalf::nvw(lv);
        const bool pk = packed_on(s);
        if (pk)  // (the gradients and -- every slot of pend is complete: the previous group's stage is ahead on this stream -- the recorded vectors)
            hipLaunchKernelGGL(k_pack_operands, dim3((unsigned)(s->n * (nvw / SMM_NV) / 32 + s->n * (np / 8) / 64)), dim3(256), 0, s->stream,
                               g_dev, s->n, lv, s->n, H.gT, H.queue, nvw / SMM_NV, (const double*)s->d_pend, s->d_pendP, np / 8);
        else
            hipLaunchKernelGGL(k_pack_grads, dim3((unsigned)((s->n * nvw + 255) / 256)), dim3(256), 0, s->stream, g_dev, s->n, lv, s->n, H.gT,
                               H.queue, nvw);
        group_pass_launch(s, {np == MAXPEND ? (int)MAXPEND : 24, nvw != SMM_NV, pk}, H, lv, s->stream, (unsigned)s->symm_wgs, s->symm_ntiles);
        HIPCHK(hipGetLastError());
    }
    owed = false;
    s->upper_stale = true;
    s->dir ^= 1;
    return pend_reset(s);
}
// an error return from a queue run leaves no apply pass owed
struct OwedGuard {
    ellhip_space* s;
    bool& owed;
    ~OwedGuard() {
        if (!owed) return;
        owed = false;
        (void)flush_pending(s, nullptr, nullptr);
    }
};

// beside: the pass is issued next to the previous group's stage -- it leaves a sixteenth of its workgroup slots free, where that
// stage's short kernels run (a pass that draws its tiles from a queue keeps every slot it gets until it ends; with a 32nd free
// k_group_sums did not get on the card before the pass ended, with an eighth the pass itself lost more than the stage gained)
int symm_go(ellhip_space* s, const double* g_dev, int lv, hipStream_t st, int half, bool beside = false, bool packed = false) {
    ProfScope ps(s, CLS_SYMV, st);
    const int wgs = beside ? std::max(1, s->symm_wgs - std::max(1, s->symm_wgs / 16)) : s->symm_wgs;
    const GroupHalf H = group_half(s, half);
    if (!packed) symm_pack_go(s, g_dev, lv, st, half);  // (packed: issued ahead of the pass already, queue_run_multi)
    group_pass_launch(s, {0, GroupHalf::nvw(lv) != SMM_NV, packed_on(s)}, H, lv, st, (unsigned)wgs, s->symm_ntiles);
    HIPCHK(hipGetLastError());
    return 0;
}

// (multi_setup: what the buffers hold before their first use, the tile list, and one empty launch of each pass)
int multi_fill(ellhip_space* s, const std::vector<SymmTile>& tiles, size_t rbytes, size_t cbytes) {
    HIPCHK(hipMemsetAsync(s->d_rowpart_m, 0, rbytes, s->stream));
    HIPCHK(hipMemsetAsync(s->d_colpart_m, 0, cbytes, s->stream));
    HIPCHK(hipMemsetAsync(s->d_gout, 0, sizeof(GroupOut), s->stream));
    if (!tiles.empty()) {
        HIPCHK(hipMemcpyAsync(s->d_symm_tiles, tiles.data(), tiles.size() * sizeof(SymmTile), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipMemsetAsync(s->d_symm_queue, 0, 256, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));  // (`tiles` is pageable host memory going out of scope)
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, s->device));
        s->symm_ntiles = (int)tiles.size();
        // two workgroups per CU is what the registers allow; more would only wait for the first ones to drain the queue
        s->symm_wgs = (int)std::min<size_t>(tiles.size(), (size_t)2 * (size_t)prop.multiProcessorCount);
        // The runtime loads a kernel at its first launch (~250 us for these): a short queue run must not meet that inside its
        // own 20 cuts because the runs before it happened to stay below 17 cuts per group.  One empty launch each (no tiles).
        // Every form this handle's group runs can take, through the runs' own launcher (group_pass_forms, group_pass_launch).
        GroupPassForm forms[12];
        const int nforms = group_pass_forms(s, forms);
        for (int k = 0; k < nforms; ++k) group_pass_launch(s, forms[k], group_half(s, 0), 0, s->stream, 1, 0);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// The group runs' buffers: 2 x 32 sets of partial sums (n^2 / 64 + n^2 / 2048 doubles each) are about n^2 doubles beside
// the matrix' n^2 (4.4 GB at n = 32768).  When they do not fit, the handle continues with one product per pass
// (returns MULTI_NO_MEMORY once; ELLHIP_OPT_LOOKAHEAD reads 1 afterwards): slower, not an error.
int multi_setup(ellhip_space* s) {
    if (s->d_rowpart_m) return 0;
    const size_t nb = (size_t)((s->n + 127) / 128);
    // two halves of MULTI_MAX sets each (and of the packed gradients): the next group's products are formed on the second
    // stream while this group's stage reads the other half
    const size_t rbytes = (size_t)2 * MULTI_MAX * rowpart_elems(s) * sizeof(double);
    const size_t cbytes = (size_t)2 * MULTI_MAX * colpart_elems(s) * sizeof(double);
    const size_t mark = s->mem.mark();
    hipError_t e = s->mem.device(s->d_rowpart_m, rbytes);
    if (e == hipSuccess) e = s->mem.device(s->d_colpart_m, cbytes);
    if (e == hipSuccess) e = s->mem.device(s->d_gT, (size_t)2 * s->n * MULTI_MAX * sizeof(double));
    if (e == hipSuccess && !s->sharded) e = s->mem.device(s->d_pendP, (size_t)MAXPEND * (size_t)s->n * sizeof(double));
    if (e == hipSuccess) e = s->mem.device(s->d_grpY, (size_t)GRP_MAX * (size_t)s->n * sizeof(double));
    if (e == hipSuccess) e = s->mem.device(s->d_gpart, (size_t)GRP_MAX * nb * (MAXPEND + 1) * sizeof(double));
    if (e == hipSuccess) e = s->mem.device(s->d_cpart, nb * GRP_MAX * GRP_MAX * sizeof(double));
    if (e == hipSuccess) e = s->mem.device(s->d_gout, sizeof(GroupOut));
    if (e == hipSuccess) e = s->mem.device(s->d_gsums, (size_t)(GRP_MAX * (MAXPEND + 1) + GRP_MAX * GRP_MAX) * sizeof(double));
    // the matrix-core pass draws its tiles from a queue, largest first (k_symm_mfma_q)
    std::vector<SymmTile> tiles;
    if ((s->n % 64) == 0 && (s->row0 % 64) == 0) {  // (whatever the lookahead is right now: the option may change)
        const long long seg = s->symv_seg;
        const long long nstrips = (s->nrows + SYMV_H - 1) / SYMV_H, nsegs = (s->n + seg - 1) / seg;
        auto blocks_of = [&](const SymmTile& t) {
            const long long r0 = s->row0 + (long long)t.I * SYMV_H, c0 = (long long)t.J * seg;
            return (std::min(c0 + seg, r0 + SYMV_H) - c0) / 16;
        };
        for (long long I = nstrips - 1; I >= 0; --I)
            for (long long J = 0; J < nsegs; ++J)
                if (J * seg <= s->row0 + I * SYMV_H + SYMV_H - 1) tiles.push_back({(int)I, (int)J});
        std::stable_sort(tiles.begin(), tiles.end(), [&](const SymmTile& a, const SymmTile& b) { return blocks_of(a) > blocks_of(b); });
        if (e == hipSuccess) e = s->mem.device(s->d_symm_tiles, tiles.size() * sizeof(SymmTile));
        if (e == hipSuccess) e = s->mem.device(s->d_symm_queue, 256);
    }
    if (e != hipSuccess) s->mem.rollback(mark);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        s->lookahead = 1;
        return MULTI_NO_MEMORY;
    }
    if (e != hipSuccess) return fail(ELLHIP_E_HIP, "buffers of the group runs", e);
    const int rc = multi_fill(s, tiles, rbytes, cbytes);
    if (rc) {  // all or nothing: d_rowpart_m, the "already set up" mark, only stays with everything behind it in place
        s->mem.rollback(mark);
        s->symm_ntiles = s->symm_wgs = 0;
    }
    return rc;
}

// (give the group runs' buffers back: the ranks of a sharded handle agreed to run cut by cut, sharded_capi.inc.hpp)
void multi_free(ellhip_space* s) {
    double** bufs[] = {&s->d_rowpart_m, &s->d_colpart_m, &s->d_gT, &s->d_pendP, &s->d_grpY, &s->d_gpart, &s->d_cpart, &s->d_gsums};
    for (double** b : bufs) s->mem.free(*b);
    s->mem.free(s->d_gout);
    s->mem.free(s->d_symm_tiles);
    s->mem.free(s->d_symm_queue);
    s->symm_ntiles = 0;
}

// the scalar stage of a group whose products sit in the partial-sum sets 2 .. 2 + g - 1 (group_kernels.hpp)
// phase 0: the reductions (they read the pass' partial sums at HBM rate and want the whole card); phase 1: the rest (Gram slices,
// sums, the one-wave recurrence, the vectors: short kernels that run beside the NEXT group's pass on the CU slots it leaves free)
template <int NP>
int group_stage_go(ellhip_space* s, long long i, int g, int half, int phase) {
    const unsigned nb = (unsigned)((s->n + 127) / 128);
    const double* grads = qgrad(s, i);
    if (phase == 0) {
        ProfScope ps(s, CLS_SYMV_REDUCE);
        const GroupHalf H = group_half(s, half);
        const double *rowp = H.rowp, *colp = H.colp;
        if (s->sharded)
            hipLaunchKernelGGL(k_group_reduce<0>, dim3(nb, (unsigned)g), dim3(256), 0, s->stream, s->n, s->row0, s->nrows,
                               (long long)s->symv_seg, rowp, colp, (long long)rowpart_elems(s), (long long)colpart_elems(s),
                               s->d_grpY, grads, s->n, (const double*)s->d_pend, s->d_gpart, (const DevState*)s->d_st);
        else if (packed_on(s))  // (the pass of this group stored its column sums in pairs)
            with_bool(group_reduce_streams(s, g), [&](auto streams) {
                constexpr int PL = decltype(streams)::value ? GROUP_REDUCE_PL_STREAM : GROUP_REDUCE_PL_CACHED;
                hipLaunchKernelGGL((k_group_reduce_p<NP, PL>), dim3(nb, (unsigned)(g + 1) / 2), dim3(256), 0, s->stream, s->n, s->row0,
                                   s->nrows, (long long)s->symv_seg, rowp, colp, (long long)rowpart_elems(s), (long long)colpart_elems(s),
                                   s->d_grpY, grads, s->n, (const double*)s->d_pend, s->d_gpart, (const DevState*)s->d_st, g, s->npend);
            });
        else
            hipLaunchKernelGGL(k_group_reduce<NP>, dim3(nb, (unsigned)g), dim3(256), 0, s->stream, s->n, s->row0, s->nrows,
                               (long long)s->symv_seg, rowp, colp, (long long)rowpart_elems(s), (long long)colpart_elems(s),
                               s->d_grpY, grads, s->n, (const double*)s->d_pend, s->d_gpart, (const DevState*)s->d_st, s->npend);
        HIPCHK(hipGetLastError());
        if (!s->sharded) return 0;
    }
    if (phase == 0) {
        // the shards' partial products become the products: ONE collective for the whole group, then the dot products from
        // the complete vectors (every rank forms the same ones)
        if (!s->grp_exchange) return fail(ELLHIP_E_STATE, "group run of a row shard without the owner's collective");
        const int xrc = s->grp_exchange(s->grp_exchange_ctx, s->d_grpY, (long long)g * s->n, s->stream);
        if (xrc) return xrc;
        ProfScope ps(s, CLS_SYMV_REDUCE);
        hipLaunchKernelGGL(k_group_dots<NP>, dim3(nb, (unsigned)g), dim3(256), 0, s->stream, s->n, (const double*)s->d_grpY, grads,
                           s->n, (const double*)s->d_pend, s->d_gpart, (const DevState*)s->d_st, s->npend);
        HIPCHK(hipGetLastError());
        return 0;
    }
    ProfScope ps(s, CLS_SCALAR);
    hipLaunchKernelGGL(k_group_gram, dim3(nb), dim3(256), 0, s->stream, s->n, g, (const double*)s->d_grpY, grads, s->n,
                       s->d_cpart, (const DevState*)s->d_st);
    hipLaunchKernelGGL(k_group_sums<NP>, dim3((unsigned)g + GRP_MAX * GRP_MAX / 256), dim3(256), 0, s->stream, g, (int)nb, (const double*)s->d_gpart,
                       (const double*)s->d_cpart, s->d_gsums, (const DevState*)s->d_st);
    hipLaunchKernelGGL(k_group_scalar<NP>, dim3(1), dim3(64), 0, s->stream, g, (const double*)s->d_gsums, s->d_cpend, s->d_st,
                       EllCalcDev::make(s->n, s->use_parallel_cut), (const CutParams*)(s->d_qparams + i), s->npend,
                       s->d_qstatus + i, s->d_qtsq + i, s->d_gout);
    hipLaunchKernelGGL(k_group_apply<NP>, dim3((unsigned)((s->n + 255) / 256)), dim3(256), 0, s->stream, s->n, g,
                       (const double*)s->d_grpY, s->d_pend, s->d_xc, s->npend, (const GroupOut*)s->d_gout);
    HIPCHK(hipGetLastError());
    return 0;
}

// ... at the recorded-update depth of the run: the group kernels' slot counts (pend / cpend hold MAXPEND)
using GroupDepths = Ints<8, 16, 24, MAXPEND>;
int bad_group_depth() { return fail(ELLHIP_E_STATE, "queue run: recorded-update depth must be 8, 16, 24 or 48"); }
int group_stage(ellhip_space* s, int qdepth, long long i, int g, int half, int phase) {
    int rc = 0;
    const bool known = with_int(GroupDepths{}, qdepth, [&](auto np) { rc = group_stage_go<decltype(np)::value>(s, i, g, half, phase); });
    return known ? rc : bad_group_depth();
}

// How many of the `rem` cuts up to the next apply pass (or the end of the run) go into the next group, `cap` = what the handle's
// lookahead and the kernels allow.  A matrix-core pass costs about the same for 4 gradients as for 16 (0.27 ms at n = 16384) and
// 0.40-0.45 for 17-32 (two column tiles over the same block of Q), so: as many as fit; and where only the 16-wide pass is allowed
// and more than one but less than two full groups are left, two even groups rather than a full one and a small one (the first
// group's stage then overlaps a pass that carries its share).
long long group_size(const ellhip_space* s, long long cap, long long rem) {
    long long g = std::min(cap, rem);
    if (multi_mfma(s) && cap <= SMM_NV && rem > cap && rem < 2 * cap) g = (rem + 1) / 2;
    return g;
}

// (the thread-to-element map, and with it the bits, follow the handle's segment width and are independent of the rows
// in flight: k_symv<8, .., 512> of the narrow segments and k_symv_multi<2, .., 512, LV> give the same sums)
template <int SEG, int LV>
void symv_multi_go(ellhip_space* s, const double* g_dev) {
    const unsigned nstrips = (unsigned)((s->nrows + SYMV_H - 1) / SYMV_H);
    const unsigned nsegs = (unsigned)((s->n + SEG - 1) / SEG);
    with_bool(s->sh_gemv.nt != 0, [&](auto ntc) {
        hipLaunchKernelGGL((k_symv_multi<2, decltype(ntc)::value, SEG, LV>), dim3(nstrips, nsegs), dim3(256), 0, s->stream,
                           (const double*)s->d_Q, s->ld, s->n, s->row0, s->nrows, g_dev, s->n, s->d_rowpart_m, s->d_colpart_m,
                           (long long)rowpart_elems(s), (long long)colpart_elems(s), (const DevState*)s->d_st);
    });
}

int queue_run_multi(ellhip_space* s, long long first, long long count) {
    int rc = multi_setup(s);
    if (rc) return rc;  // (MULTI_NO_MEMORY: the caller goes on with the schedules that need no extra buffers)
    const long long end = first + count;
    if (s->sharded && (s->primed || !s->grp_exchange))
        return fail(ELLHIP_E_STATE, "group run of a row shard: the owner takes a primed cut by itself and supplies the collective");
    // Inside this run the group stage may let more updates pile up than the handle's depth (its kernels are sized for
    // MAXPEND = 48; the per-cut kernels of every other path for the depth): half as many apply passes.  Whatever leaves
    // this function has fewer recorded than the depth again.
    const bool deep_ok = multi_mfma(s) && s->defer == 24 && s->apply_lower && s->queue_depth > s->defer;
    const int qdepth = deep_ok ? s->queue_depth : s->defer;
    if (!with_int(GroupDepths{}, qdepth, [](auto) {})) return bad_group_depth();
    // (round 3, the pass beside the whole stage: +1.5 % / +8 % at n = 16384 for 200 / 20 cuts per run, -3 % at n = 32768, so the
    // second stream stopped at n = 24576.  Round 4, the pass behind the stage's reductions and beside the rest of it on the slots
    // it leaves free: +6 % at n = 16384 (200 cuts), +1.5 % at n = 32768 -- used at every size)
    const bool use_side = multi_mfma(s) && s->overlap != 0 && !s->sharded;
    if (use_side) {
        rc = side_setup(s);
        if (rc) return rc;
    }
    SideGuard guard{s};
    // ELLHIP_OPT_APPLY_SYMM: when a group fills the slots and another group follows inside this run, the apply pass stays owed
    // and the next trip issues it fused with that group's products (k_apply_symm_q).  Not when that group ends the run: the
    // run's last group keeps the separate passes (and the launch counts the suite pins for groups of 32, 16 | 8).
    bool owed = false;
    OwedGuard oguard{s, owed};
    int half = 0;                       // the half of the partial-sum sets the current group's products are in
    long long ahead_i = -1, ahead_g = 0;  // the group whose products are in flight on the second stream
    long long i = first;
    while (i < end) {
        long long g = 1;
        if (!(s->primed && s->primed_qindex == i)) {
            rc = ensure_committed(s);
            if (rc) return rc;
            const long long room = (long long)qdepth - (owed ? 0 : s->npend);  // cuts that can still be recorded before the apply pass
            const long long cap = std::min<long long>(s->lookahead, multi_mfma(s) ? MULTI_MAX : MULTI_VALU_MAX);
            const long long rem = std::min(end - i, room);  // cuts up to the next apply pass or the end of the run
            g = group_size(s, cap, rem);
        }
        if (g <= 1 && !s->sharded) {  // a cut primed earlier, the last one before an apply pass, the last one of the run
            if (s->npend >= s->defer) {  // (the per-cut kernels hold `depth` recorded updates)
                owed = false;
                rc = flush_pending(s, nullptr, nullptr);
                if (rc) return rc;
            }
            rc = queue_prime_impl(s, i);
            if (!rc) rc = queue_cut_impl(s, i);
            if (!rc) rc = queue_commit_impl(s, i, -1);
            if (rc) return rc;
            i += 1;
            continue;
        }
        if (multi_mfma(s)) {
            const long long cap = MULTI_MAX;
            rc = side_join(s);  // (this group's products, when they were issued ahead)
            if (rc) return rc;
            if (owed) {  // (nothing was issued ahead: the previous group filled the slots)
                rc = apply_symm_go(s, qgrad(s, i), (int)g, half, apply_symm_np(s), owed);
                if (rc) return rc;
            } else if (!(ahead_i == i && ahead_g == g)) {  // this group's products are not in the sets yet
                rc = symm_go(s, qgrad(s, i), (int)g, s->stream, half);
                if (rc) return rc;
            }
            ahead_i = -1;
            // the NEXT group's products on the second stream beside this group's stage -- when there is one inside this run
            // and no apply pass comes first (it would read the matrix that pass writes)
            const long long i2 = i + g, room2 = (long long)qdepth - (s->npend + g);
            long long g2 = 0;
            if (i2 < end && room2 > 0) {
                const long long cap2 = std::min<long long>(s->lookahead, cap), rem2 = std::min(end - i2, room2);
                g2 = group_size(s, cap2, rem2);  // (the rule the next trip of the loop applies)
            }
            // the whole group's scalar stage: the cuts' omegas and coefficients from dot products that exist when the group
            // starts, then the vectors in one elementwise pass.  First its reductions (they stream the pass' partial sums and want
            // the whole card) ...
            drop_prime(s);
            s->dots_np = 0;
            s->xc_host_valid = false;
            // (the NEXT group's operands first, on the second stream: they go into the other half of gT and rewind its tile counter,
            // whose last reader is the pass that ran on that half one group earlier -- enqueued on, or joined into, the handle's
            // stream by now, so the fork covers it.  Only the pass itself waits for the reductions.)
            const bool go_side = use_side && g2 >= 2;
            if (go_side) {
                rc = side_fork(s);
                if (rc) return rc;
                symm_pack_go(s, qgrad(s, i2), (int)g2, side_stream(s), half ^ 1);
                HIPCHK(hipGetLastError());
            }
            rc = group_stage(s, qdepth, i, (int)g, half, 0);
            if (rc) {
                if (go_side) (void)side_mark(s);  // (the operands' launch is side work in flight: the guard joins it)
                return rc;
            }
            // ... then the NEXT group's products on the second stream, behind those reductions and beside the rest of this
            // stage (short kernels, one of them a single wave: they run on the slots the pass leaves free)
            if (go_side) {
                rc = side_fork(s);  // after this group's reductions: the last reader of the other half, every writer of Q so far
                if (!rc) rc = symm_go(s, qgrad(s, i2), (int)g2, side_stream(s), half ^ 1, true, true);
                if (!rc) rc = side_mark(s);
                if (rc) return rc;
                ahead_i = i2;
                ahead_g = g2;
            }
            rc = group_stage(s, qdepth, i, (int)g, half, 1);
            if (rc) return rc;
            s->npend += (int)g;       // (optimistic, as after every queue cut: ellhip_queue_results settles it after a halt)
            s->scalars_stale = true;
            s->shrink_pending = false;
            if (s->npend >= qdepth) {
                const long long in = i + g;
                long long gn = 0;  // the next group, sized as the loop head will size it once the slots are free
                if (in < end && apply_symm_np(s) != 0)
                    gn = group_size(s, std::min<long long>(s->lookahead, MULTI_MAX), std::min<long long>(end - in, qdepth));
                if (gn >= 2 && in + gn < end) {
                    owed = true;
                } else {
                    rc = flush_pending(s, nullptr, nullptr);
                    if (rc) return rc;
                }
            }
            if (ahead_i >= 0) half ^= 1;
            i += g;
            continue;
        }
        {
            ProfScope ps(s, CLS_SYMV);
            with_bool(s->symv_seg == SYMV_SEG, [&](auto wide) {
                constexpr int SEG = decltype(wide)::value ? SYMV_SEG : SYMV_SEG_SMALL;
                if (g == 2) symv_multi_go<SEG, 2>(s, qgrad(s, i));
                else symv_multi_go<SEG, 3>(s, qgrad(s, i));
            });
            HIPCHK(hipGetLastError());
        }
        for (long long l = 0; l < g; ++l) {
            s->part_set = 2 + (int)l;
            s->dots_np = 0;
            s->dots_need_gy = false;
            rc = launch_symv_reduce(s, qgrad(s, i + l), s->d_gt[s->cur]);
            s->part_set = 0;
            if (rc) return rc;
            s->primed = true;
            s->g_cur = qgrad(s, i + l);
            s->primed_qindex = i + l;
            rc = queue_cut_impl(s, i + l);
            if (!rc) rc = queue_commit_impl(s, i + l, -1);  // (the apply pass when this cut fills the slots)
            if (rc) return rc;
        }
        i += g;
    }
    if (s->npend >= s->defer) return flush_pending(s, nullptr, nullptr);
    return 0;
}

}  // namespace
