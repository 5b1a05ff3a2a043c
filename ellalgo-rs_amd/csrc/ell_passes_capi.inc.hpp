// ell_passes_capi.inc.hpp -- the passes over Q of an Ell handle: which schedule is in force (deferring, symv_ok), the launch
// shapes (pick_shape), the full-row sweeps (k_sweep, k_sweep_gemv_dots), the apply passes of the recorded schedule
// (flush_pending: k_sweep_apply, k_apply_lower, k_apply_mfma), the one-off mirror, and the lower-triangle GEMV with its
// partial-sum sets (symv_alloc, launch_symv_tiles, launch_symv_reduce).  One function per kernel family builds the argument
// list; launch_dispatch.hpp turns the run-time shape into template arguments.
// Needs: ell_handle_capi.inc.hpp, ell_side_capi.inc.hpp, launch_dispatch.hpp.  DESIGN.md sections 3.1, 3.3, 3.4.

namespace {

// Deferred mode is in force for Ell with depth > 1, except while the reference semantics need Q itself
// to be rewritten at once (no_defer_trick scaling; the one-off mirror of a non-symmetric input).
bool deferring(const ellhip_space* s) {
    return s->variant == ELLHIP_SPACE_ELL && s->defer > 1 && !s->no_defer_trick && !s->needs_mirror;
}

// Lower-triangle GEMV: deferred mode (Q_base is bit-symmetric and only read).  Unsharded handles from
// symv_min_n up; a row shard only in its symmetric mode (ellhip_set_shard_symmetric), where the GEMV yields this
// shard's PARTIAL sums over its lower trapezoid and the caller adds the shards' vectors (all-reduce).
bool symv_ok(const ellhip_space* s) {
    if (!(deferring(s) && s->symv && (s->n % 2) == 0 && s->d_rowpart)) return false;
    return s->sharded ? s->shard_symmetric : s->n >= s->symv_min_n;
}

// ---- launch-shape selection ------------------------------------------------------------------
// A workgroup covers RW rows; each lane keeps RW*UNR 16-byte loads in flight.  Defaults come from
// in-process A/B sweeps on MI355X (tools/tune_ell.hip, numbers in DESIGN.md / profiles/):
//   * local Q block fits the 256 MiB Infinity Cache (n = 4096: 128 MiB): keep the default cache
//     policy so the next pass finds Q on-die;
//   * larger: the Q stream is touched once per pass, so use the non-temporal policy (GEMV pass 4.9 ->
//     7.0 TB/s at n = 16384).
void pick_shape(ellhip_space* s) {
    const double q_bytes = (double)s->nrows * (double)s->ld * 8.0;
    const double MiB = 1024.0 * 1024.0;
    if (q_bytes <= 200.0 * MiB) {          // lives in the Infinity Cache between passes
        s->sh_gemv = {4, 2, 0};
        s->sh_rank1 = {4, 4, 0};
        s->sh_fused = {4, 4, 0};
    } else if (q_bytes <= 1024.0 * MiB) {  // a few x the cache: read-only pass streams, RMW passes keep what fits
        s->sh_gemv = {4, 4, 1};
        s->sh_rank1 = {4, 4, 0};
        s->sh_fused = {4, 4, 0};
    } else {                               // pure streaming
        s->sh_gemv = {4, 4, 1};
        s->sh_rank1 = {2, 8, 1};
        s->sh_fused = {2, 8, 1};
    }
    s->sh_apply = {4, 1, s->sh_fused.nt};  // 8 pending vectors per column step: more rows per workgroup amortise them
    static_cast<SpaceOptions&>(*s) = g_defaults;  // (what a new handle starts with)
}

// ---- from the run-time shape to a kernel: the lists each family is built for ---------------------------------------------------
template <int RW, int UNR>
struct RowsUnroll { static constexpr int rw = RW, unr = UNR; };
using SweepShapes = OneOf<RowsUnroll<1, 4>, RowsUnroll<1, 8>, RowsUnroll<2, 4>, RowsUnroll<2, 8>, RowsUnroll<4, 2>, RowsUnroll<4, 4>,
                          RowsUnroll<8, 1>, RowsUnroll<8, 2>>;  // k_sweep, k_sweep_gemv_dots
using ApplyShapes = OneOf<RowsUnroll<1, 2>, RowsUnroll<1, 4>, RowsUnroll<2, 1>, RowsUnroll<2, 2>, RowsUnroll<2, 4>, RowsUnroll<4, 1>,
                          RowsUnroll<4, 2>>;                    // k_sweep_apply
template <class List, class F>
bool with_shape(List, const Shape& sh, F&& f) {  // false: the list has no such RW x UNR
    return with_one_of(List{}, [&](auto c) { return sh.rw == decltype(c)::rw && sh.unr == decltype(c)::unr; }, f);
}
// (VEC, NT) of a full-row pass: odd n has rows that are not 16-byte aligned and takes 8-byte accesses, never non-temporal
// ones -- three forms, there is no (1, true)
using Vec1 = std::integral_constant<int, 1>;
using Vec2 = std::integral_constant<int, 2>;
template <class F>
bool with_access(const ellhip_space* s, const Shape& sh, F&& f) {
    if ((s->n % 2) != 0) return f(Vec1{}, std::false_type{});
    return sh.nt ? f(Vec2{}, std::true_type{}) : f(Vec2{}, std::false_type{});
}
constexpr const char* BAD_SWEEP_SHAPE = "unsupported RW/UNR launch shape (supported: 1x4 1x8 2x4 2x8 4x2 4x4 8x1 8x2)";

// One pass over Q in the given roles.  gt_r1: vector of the rank-1 role; gvec / gv_out: operand and
// result of the GEMV role (gv_out is the full-length buffer; the shard's rows start at row0).
template <bool R1, bool GV>
int launch_sweep(ellhip_space* s, const Shape& sh, const double* gt_r1, const double* gvec, double* gv_out) {
    const long long nr = s->nrows;
    const unsigned grid = (unsigned)((nr + sh.rw - 1) / sh.rw);
    double* out = gv_out ? gv_out + s->row0 : nullptr;
    const bool known = with_access(s, sh, [&](auto vec, auto nt) {
        return with_bool(R1 && s->no_defer_trick, [&](auto scale) {
            return with_shape(SweepShapes{}, sh, [&](auto c) {
                hipLaunchKernelGGL((k_sweep<decltype(c)::rw, decltype(c)::unr, decltype(vec)::value, decltype(nt)::value, R1, GV,
                                            R1 && decltype(scale)::value>),
                                   dim3(grid), dim3(256), 0, s->stream, (const double*)s->d_Q, s->d_Q, s->ld, s->n, nr, s->row0, gt_r1,
                                   gvec, out, s->d_st, s->dir);
            });
        });
    });
    if (!known) return fail(ELLHIP_E_INVALID, BAD_SWEEP_SHAPE);
    HIPCHK(hipGetLastError());
    s->dir ^= 1;  // the next pass over Q runs the other way
    return 0;
}

// Full-row GEMV of the deferred schedule with the v_j . g dot products computed beside it (k_sweep_gemv_dots).
int launch_gemv_dots(ellhip_space* s, const double* gvec, double* gv_out) {
    const Shape& sh = s->sh_gemv;
    const long long nr = s->nrows;
    const unsigned ntiles = (unsigned)((nr + sh.rw - 1) / sh.rw);
    const unsigned grid = ntiles + (unsigned)scalar_groups(s->n);
    const bool known = with_access(s, sh, [&](auto vec, auto nt) {
        return with_shape(SweepShapes{}, sh, [&](auto c) {
            hipLaunchKernelGGL((k_sweep_gemv_dots<decltype(c)::rw, decltype(c)::unr, decltype(vec)::value, decltype(nt)::value, 8>),
                               dim3(grid), dim3(256), 0, s->stream, (const double*)s->d_Q, s->ld, s->n, nr, s->row0, gvec,
                               gv_out + s->row0, s->d_st, s->dir, ntiles, (const double*)s->d_pend, s->d_partial);
        });
    });
    if (!known) return fail(ELLHIP_E_INVALID, BAD_SWEEP_SHAPE);
    HIPCHK(hipGetLastError());
    s->dir ^= 1;
    s->dots_np = 8;
    s->dots_need_gy = true;
    return 0;
}

// ---- the apply passes of the recorded schedule: one launcher per kernel -------------------------------------------------------
// k_sweep_apply: full rows, optionally with the GEMV of gvec; LOWER: the lower triangle only (even n: VEC = 2)
template <bool GV, bool LOWER, class VecC, class NtC>
bool launch_sweep_apply(ellhip_space* s, const double* gvec, double* gv_out, VecC, NtC) {
    const Shape& sh = s->sh_apply;
    const long long nr = s->nrows;
    const unsigned grid = (unsigned)((nr + sh.rw - 1) / sh.rw);
    double* out = gv_out ? gv_out + s->row0 : nullptr;
    const int dir = LOWER ? 1 : s->dir;  // lower-only: last (longest) rows first, so the short ones fill the tail
    return with_shape(ApplyShapes{}, sh, [&](auto c) {
        hipLaunchKernelGGL((k_sweep_apply<decltype(c)::rw, decltype(c)::unr, VecC::value, NtC::value, GV, LOWER>), dim3(grid), dim3(256), 0,
                           s->stream, (const double*)s->d_Q, s->d_Q, s->ld, s->n, nr, s->row0, (const double*)s->d_pend,
                           (const double*)s->d_cpend, gvec, out, s->d_st, dir);
    });
}
// the lower triangle alone, on the matrix cores (k_apply_mfma: the rank-NP update; 8, 16, 24 or -- what a queue run on the group
// stage let pile up -- 48 recorded updates) or in 16-row tiles with the coefficients in LDS (k_apply_lower: 8, 16 or 24)
void launch_apply_lower(ellhip_space* s, bool mfma, int np, bool nt) {
    auto go = [&](auto kernel, dim3 grid) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s->stream, s->d_Q, s->ld, s->n, s->nrows, s->row0, (const double*)s->d_pend,
                           (const double*)s->d_cpend, (const DevState*)s->d_st);
    };
    const dim3 tiles((unsigned)((s->nrows + APM_ROWS - 1) / APM_ROWS), (unsigned)((s->n + APM_COLS - 1) / APM_COLS));
    with_bool(nt, [&](auto ntc) {
        constexpr bool NT = decltype(ntc)::value;
        if (mfma) with_int(Ints<8, 16, 24, MAXPEND>{}, np, [&](auto npc) { go(k_apply_mfma<decltype(npc)::value, NT>, tiles); });
        else with_int(Ints<8, 16, 24>{}, np, [&](auto npc) { go(k_apply_lower<decltype(npc)::value, NT>, dim3((unsigned)((s->nrows + APL_TR - 1) / APL_TR))); });
    });
}

// (after an apply pass: forget the recorded updates)
int pend_reset(ellhip_space* s) {
    hipLaunchKernelGGL(k_pend_reset, dim3(64), dim3(256), 0, s->stream, s->d_pend, s->d_cpend,
                       (long long)(s->npend > s->defer ? MAXPEND : s->defer) * s->n, s->d_st);
    HIPCHK(hipGetLastError());
    s->npend = 0;
    return 0;
}
// Apply every pending update to Q (one pass), optionally fused with the GEMV of `gvec`; then clear the slots.
// While the GEMVs of this handle read the lower triangle only (symv_ok), so does the apply pass: half the
// traffic; the strict upper triangle goes stale until make_q_current() mirrors it back.
int flush_pending(ellhip_space* s, const double* gvec, double* gv_out) {
    {
        int jrc = side_join(s);  // a writer of Q: nothing issued ahead on the second stream may still be reading it
        if (jrc) return jrc;
        ProfScope ps(s, gvec ? CLS_APPLY_GEMV : CLS_APPLY);
        const bool lower = !gvec && s->apply_lower && symv_ok(s);
        bool known = true;
        if (lower) {
            // measured at n = 16384, ms per pass: k_apply_mfma 0.43-0.44 at any depth; k_apply_lower 0.40 at depth 8 / 16,
            // 0.62 at depth 24 (its registers); k_sweep_apply<LOWER> 0.44 (depth 8)
            // (more recorded than the handle's depth: a queue run on the group stage let them pile up to 48, queue_run_multi)
            const bool deep = s->npend > s->defer;
            const int apply_kernel = deep ? 2 : (s->apply_kernel < 0 ? (s->defer == 24 ? 2 : 1) : s->apply_kernel);
            const int np = deep ? MAXPEND : (s->defer == 24 || s->defer == 16) ? s->defer : 8;
            const bool nt = s->sh_apply.nt != 0;
            // (k_sweep_apply holds 8 recorded updates: at depth 16 / 24 ELLHIP_OPT_APPLY_KERNEL = 0 takes k_apply_lower as 1 does)
            if (apply_kernel != 0 || np > 8) launch_apply_lower(s, apply_kernel == 2, np, nt);
            else known = with_bool(nt, [&](auto ntc) { return launch_sweep_apply<false, true>(s, nullptr, nullptr, Vec2{}, ntc); });
        } else if (s->defer != 8) {
            return fail(ELLHIP_E_STATE, "defer depth 16 / 24 needs the lower-triangle schedule");
        } else {
            known = with_bool(gvec != nullptr, [&](auto gv) {
                return with_access(s, s->sh_apply, [&](auto vec, auto ntc) {
                    return launch_sweep_apply<decltype(gv)::value, false>(s, gvec, gv_out, vec, ntc);
                });
            });
        }
        if (!known) return fail(ELLHIP_E_INVALID, "unsupported ELLHIP_APPLY_RW/UNR shape (supported: 1x2 1x4 2x1 2x2 2x4 4x1 4x2)");
        if (lower) s->upper_stale = true;
        HIPCHK(hipGetLastError());
        s->dir ^= 1;
    }
    return pend_reset(s);
}

int launch_mirror_if_needed(ellhip_space* s) {
    if (!s->needs_mirror) return 0;
    const unsigned t = (unsigned)((s->n + 31) / 32);
    hipLaunchKernelGGL(k_mirror_lower, dim3(t, t), dim3(256), 0, s->stream, s->d_Q, s->ld, s->n, s->d_st);
    HIPCHK(hipGetLastError());
    return 0;
}

// One set of partial sums of the lower-triangle GEMV, zeroed on the handle's stream: both buffers or neither
// (rows of rowpart outside a shard are never written but are read by nobody either; they are zeroed anyway)
int part_pair_alloc(ellhip_space* s, double*& rowpart, double*& colpart, size_t rbytes, size_t cbytes) {
    const size_t mark = s->mem.mark();
    hipError_t e = s->mem.device(rowpart, rbytes);
    if (e == hipSuccess) e = s->mem.device(colpart, cbytes);
    if (e == hipSuccess) e = hipMemsetAsync(rowpart, 0, rbytes, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(colpart, 0, cbytes, s->stream);
    if (e == hipSuccess) return 0;
    s->mem.rollback(mark);
    return fail(ELLHIP_E_HIP, "partial-sum set of the lower-triangle GEMV", e);
}

int symv_alloc(ellhip_space* s) {
    if (s->d_rowpart || (s->n % 2) != 0 || s->n < 512 || (s->sharded && !s->shard_symmetric)) return 0;
    // tiles of 64 x 2048 in this handle's lower trapezoid; with fewer than ~200 (less than one per CU) the narrow
    // segments win (measured per rank at n = 16384: P = 8, 128 tiles: 0.049 vs 0.061 ms; P = 4, 256 tiles: 0.078 vs
    // 0.067; P = 2: 0.109 vs 0.104; unsharded n = 8192, 256 tiles: 0.076 vs 0.066)
    const double area = ((double)(s->row0 + s->nrows) * (double)(s->row0 + s->nrows) - (double)s->row0 * (double)s->row0) / 2.0;
    const int seg = (area / (64.0 * SYMV_SEG) < 200.0) ? SYMV_SEG_SMALL : SYMV_SEG;
    const size_t nsegs = (size_t)((s->n + seg - 1) / seg), nstrips = (size_t)((s->nrows + SYMV_H - 1) / SYMV_H);
    const int rc = part_pair_alloc(s, s->d_rowpart, s->d_colpart, nsegs * (size_t)s->n * sizeof(double), nstrips * (size_t)s->n * sizeof(double));
    if (rc) return rc;
    s->symv_seg = seg;
    // rows in flight per thread: with about one 64 x 2048 tile per CU (n = 8192: 256 tiles) the workgroup itself has to
    // keep more loads in the air -- 4 rows: 61 vs 65 us per pass; with several tiles per CU (n = 16384) 2 and 4 tie
    s->symv_rw = (area / (64.0 * SYMV_SEG) < 600.0) ? 4 : 2;
    return 0;
}

// partial-sum sets of the lower-triangle GEMV: 0 = the handle's own, 1 = the second set of overlapped queue runs,
// 2 + l = vector l of a k_symv_multi group
constexpr int MULTI_MAX = 32;  // = GRP_MAX = 2 * SMM_NV: gradients per matrix-core pass at most
constexpr int MULTI_VALU_MAX = 3;  // largest group k_symv_multi takes (vector ALU, bit-identical to k_symv)
size_t rowpart_elems(const ellhip_space* s) { return (size_t)((s->n + s->symv_seg - 1) / s->symv_seg) * (size_t)s->n; }
size_t colpart_elems(const ellhip_space* s) { return (size_t)((s->nrows + SYMV_H - 1) / SYMV_H) * (size_t)s->n; }
double* rowpart_of(const ellhip_space* s, int set) {
    return set == 0 ? s->d_rowpart : set == 1 ? s->d_rowpart2 : s->d_rowpart_m + (size_t)(set - 2) * rowpart_elems(s);
}
double* colpart_of(const ellhip_space* s, int set) {
    return set == 0 ? s->d_colpart : set == 1 ? s->d_colpart2 : s->d_colpart_m + (size_t)(set - 2) * colpart_elems(s);
}

template <int RW, int SEG>
void symv_go(ellhip_space* s, const double* g_dev, unsigned nstrips, unsigned nsegs, bool nt, hipStream_t st, int set) {
    with_bool(nt, [&](auto ntc) {
        hipLaunchKernelGGL((k_symv<RW, decltype(ntc)::value, 0, SEG>), dim3(nstrips, nsegs), dim3(256), 0, st, (const double*)s->d_Q,
                           s->ld, s->n, s->row0, s->nrows, g_dev, rowpart_of(s, set), colpart_of(s, set), s->d_st);
    });
}

// the reduction of the tiles launch_symv has issued (by itself: k_symv_reduce<NP>)
int launch_symv_reduce(ellhip_space* s, const double* g_dev, double* y_out) {
    const int seg = s->symv_seg;
    ProfScope ps(s, CLS_SYMV_REDUCE);
    // unsharded: the reduction also yields the scalar stage's dot products (a shard's y is partial until the owner's
    // all-reduce has run, so its dot products wait for k_scalar_dot_def)
    const int np = (!s->sharded && s->fuse_dots) ? s->defer : 0;
    auto go = [&](auto npc) {
        hipLaunchKernelGGL(k_symv_reduce<decltype(npc)::value>, dim3((unsigned)((s->n + 127) / 128)), dim3(256), 0, s->stream, s->n,
                           s->row0, s->nrows, (long long)seg, (const double*)rowpart_of(s, s->part_set),
                           (const double*)colpart_of(s, s->part_set), y_out, s->d_st, g_dev, (const double*)s->d_pend, s->d_partial);
    };
    if (!with_int(Ints<0, 8, 16, 24>{}, np, go)) go(std::integral_constant<int, 0>{});  // (any other depth: the sums alone)
    HIPCHK(hipGetLastError());
    s->dots_np = np;
    return 0;
}

// the tiles alone, on `st`, into partial-sum set `set`
int launch_symv_tiles(ellhip_space* s, const double* g_dev, hipStream_t st, int set) {
    const int seg = s->symv_seg;
    ProfScope ps(s, CLS_SYMV, st);
    const unsigned nstrips = (unsigned)((s->nrows + SYMV_H - 1) / SYMV_H);  // local strips
    const unsigned nsegs = (unsigned)((s->n + seg - 1) / seg);
    const bool nt = s->sh_gemv.nt != 0;
    if (seg == SYMV_SEG_SMALL) {
        symv_go<8, SYMV_SEG_SMALL>(s, g_dev, nstrips, nsegs, nt, st, set);  // narrow segments: 8 rows x 1 chunk in flight
    } else if (seg == SYMV_SEG) {
        if (!with_int(Ints<1, 2, 4, 8>{}, s->symv_rw, [&](auto rw) { symv_go<decltype(rw)::value, SYMV_SEG>(s, g_dev, nstrips, nsegs, nt, st, set); }))
            return fail(ELLHIP_E_INVALID, "unsupported rows-in-flight of the lower-triangle GEMV (1, 2, 4, 8)");
    } else {
        return fail(ELLHIP_E_INVALID, "unsupported segment width of the lower-triangle GEMV (512, 2048)");
    }
    HIPCHK(hipGetLastError());
    return 0;
}
int launch_symv(ellhip_space* s, const double* g_dev, double* y_out) {
    const int rc = launch_symv_tiles(s, g_dev, s->stream, s->part_set);
    return rc ? rc : launch_symv_reduce(s, g_dev, y_out);
}

}  // namespace
