// ell_options_capi.inc.hpp -- the option table (one row per ELLHIP_OPT_* key) and the four entry points that read nothing
// else: ellhip_set_default_option, ellhip_default_option, ellhip_set_option, ellhip_get_option (C linkage from
// include/ellhip.h).  Needs: ell_handle_capi.inc.hpp (SpaceOptions, Defaults), ell_primitives_capi.inc.hpp (make_q_current).
// DESIGN.md section 13.

// ---- options ----------------------------------------------------------------------------------
// One row per ELLHIP_OPT_* key: the four entry points below read nothing else.  A new option is a field of SpaceOptions
// (or of Defaults, when it exists as a default only) and a row here.
namespace {
enum OptWho : unsigned char { OPT_DEFAULT_ONLY, OPT_ELL, OPT_STABLE, OPT_READ_ONLY };  // who may set it (on a handle: Ell / EllStable only)
// what ellhip_set_option does first: nothing (read per queue run); make Q current (what has been recorded, and a stale upper
// triangle, belong to the schedule in force); leave the mirrored layout (the next update enters the layout its options ask for)
enum OptFirst : unsigned char { FIRST_NOTHING, FIRST_Q_CURRENT, FIRST_LEAVE_MIRROR };
constexpr long long OPT_NO_MAX = 0x7fffffffffffffffLL;
struct OptAllowed {  // a range lo .. hi (empty: nothing may be stored), or (nset > 0) a set
    long long lo, hi;
    int nset;
    long long set[4];
};
constexpr OptAllowed range(long long lo, long long hi) { return {lo, hi, 0, {}}; }
constexpr OptAllowed at_least(long long lo) { return {lo, OPT_NO_MAX, 0, {}}; }
struct OptionRow {
    int key;
    const char* name;
    long long SpaceOptions::*opt;  // where the value lives: a per-handle option (in every handle and in g_defaults),
    long long* def_only;           // a default-only value (in g_defaults), or neither (per-handle state outside the record)
    OptAllowed allowed;
    OptWho who;
    OptFirst first;
};
#define OPT_ROW(KEY, FIELD, ...) {ELLHIP_OPT_##KEY, "ELLHIP_OPT_" #KEY, &SpaceOptions::FIELD, nullptr, __VA_ARGS__}
#define OPT_DEF(KEY, FIELD, ...) {ELLHIP_OPT_##KEY, "ELLHIP_OPT_" #KEY, nullptr, &g_defaults.FIELD, __VA_ARGS__, OPT_DEFAULT_ONLY, FIRST_NOTHING}
#define OPT_OWN(KEY, ...) {ELLHIP_OPT_##KEY, "ELLHIP_OPT_" #KEY, nullptr, nullptr, __VA_ARGS__, FIRST_NOTHING}
const OptionRow g_option_table[] = {
    OPT_DEF(AUTO_DEFER, auto_defer, range(0, 1)),
    OPT_ROW(SYMV, symv, range(0, 1), OPT_ELL, FIRST_Q_CURRENT),
    OPT_ROW(SYMV_MIN_N, symv_min_n, at_least(512), OPT_ELL, FIRST_Q_CURRENT),
    OPT_ROW(APPLY_LOWER, apply_lower, range(0, 1), OPT_ELL, FIRST_Q_CURRENT),
    OPT_ROW(APPLY_KERNEL, apply_kernel, range(-1, 2), OPT_ELL, FIRST_Q_CURRENT),
    OPT_ROW(FUSE_DOTS, fuse_dots, range(0, 1), OPT_ELL, FIRST_Q_CURRENT),
    OPT_ROW(STABLE_SOLVE, stable_solve, range(0, 3), OPT_STABLE, FIRST_LEAVE_MIRROR),
    OPT_ROW(STABLE_FACTOR, stable_factor, range(0, 2), OPT_STABLE, FIRST_LEAVE_MIRROR),
    OPT_DEF(PAD, pad, range(-1, 4096)),
    OPT_DEF(LP_GRID, lp_grid, range(0, 65536)),
    OPT_DEF(LP_WIDE, lp_wide, range(-1, 1)),
    OPT_DEF(BATCH_THREADS, batch_threads, {0, 0, 4, {0, 64, 128, 256}}),
    OPT_ROW(RESIDENT, resident, range(0, 2), OPT_ELL, FIRST_NOTHING),
    OPT_ROW(OVERLAP, overlap, range(0, 2), OPT_ELL, FIRST_NOTHING),
    OPT_ROW(LOOKAHEAD, lookahead, range(1, 32), OPT_ELL, FIRST_NOTHING),
    OPT_ROW(QUEUE_DEPTH, queue_depth, {0, 0, 2, {0, 48}}, OPT_ELL, FIRST_NOTHING),
    OPT_OWN(RESIDENT_FAULT, at_least(-1), OPT_ELL),  // ellhip_space::rs_fault_at: per handle only, not inherited by a clone
    OPT_OWN(RESIDENT_ABANDONED, range(0, -1), OPT_READ_ONLY),
    OPT_OWN(STABLE_MIRRORED, range(0, -1), OPT_READ_ONLY),
    OPT_DEF(STAGE_DIRECT, stage_direct, range(0, 1)),  // (per handle: read only, what alloc_common decided)
    OPT_ROW(APPLY_SYMM, apply_symm, range(0, 1), OPT_ELL, FIRST_NOTHING),
    OPT_ROW(PACKED_OPERANDS, packed_operands, range(0, 1), OPT_ELL, FIRST_NOTHING),
};
#undef OPT_ROW
#undef OPT_DEF
#undef OPT_OWN

const OptionRow* option_row(int key) {
    for (const OptionRow& r : g_option_table)
        if (r.key == key) return &r;
    (void)fail(ELLHIP_E_INVALID, "unknown option key");
    return nullptr;
}
long long* option_slot(ellhip_space* s, const OptionRow& r) {  // where a handle keeps the row's value (NULL: it keeps none)
    return r.opt ? &(s->*r.opt) : r.key == ELLHIP_OPT_RESIDENT_FAULT ? &s->rs_fault_at : nullptr;
}
int option_refuse(const OptionRow& r, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", r.name, why);
    return fail(ELLHIP_E_INVALID, buf);
}
long long* default_slot(const OptionRow* r) {  // where g_defaults keeps it (NULL, message set: unknown key, or per handle only)
    if (r && !r->opt && !r->def_only) (void)option_refuse(*r, "not a creation-time default (per handle only)");
    return !r ? nullptr : r->opt ? &(g_defaults.*r->opt) : r->def_only;
}
int option_value_ok(const OptionRow& r, long long v) {
    const OptAllowed& a = r.allowed;
    char what[128] = "read only";
    int len = 0;
    for (int i = 0; i < a.nset; ++i) {
        if (a.set[i] == v) return 0;
        len += snprintf(what + len, sizeof what - (size_t)len, i ? ", %lld" : "value must be one of %lld", a.set[i]);
    }
    if (a.nset == 0 && v >= a.lo && v <= a.hi) return 0;
    if (a.nset == 0 && a.hi == OPT_NO_MAX) snprintf(what, sizeof what, "value must be >= %lld", a.lo);
    else if (a.nset == 0 && a.lo <= a.hi) snprintf(what, sizeof what, "value must be in %lld .. %lld", a.lo, a.hi);
    return option_refuse(r, what);
}
// FIRST_Q_CURRENT, after the value is in place: a lowered threshold may bring the lower-triangle schedule into reach;
// depth 16 / 24 exist on that schedule only, so where it is gone the handle falls back to depth 8
int option_schedule_changed(ellhip_space* s) {
    if (s->defer > 1) {
        const int rc = symv_alloc(s);
        if (rc) return rc;
    }
    if (s->defer >= 16) {
        const bool lower = s->symv && s->apply_lower && (s->n % 2) == 0 && s->d_rowpart &&
                           (s->sharded ? s->shard_symmetric : s->n >= s->symv_min_n);
        if (!lower) s->defer = 8;
    }
    return 0;
}
}  // namespace

int ellhip_set_default_option(int key, int64_t value) {
    const OptionRow* r = option_row(key);
    long long* slot = default_slot(r);
    if (!slot) return ELLHIP_E_INVALID;
    const int rc = option_value_ok(*r, value);
    if (!rc) *slot = value;
    return rc;
}

int ellhip_default_option(int key, int64_t* value) {
    if (!value) return fail(ELLHIP_E_INVALID, "value is NULL");
    const long long* slot = default_slot(option_row(key));
    if (!slot) return ELLHIP_E_INVALID;
    *value = *slot;
    return 0;
}

int ellhip_set_option(ellhip_space* s, int key, int64_t value) {
    if (!s) return fail(ELLHIP_E_INVALID, "NULL handle");
    const OptionRow* r = option_row(key);
    if (!r) return ELLHIP_E_INVALID;
    int rc = option_value_ok(*r, value);
    if (rc) return rc;
    DeviceGuard guard(s->device);
    const bool ell = s->variant == ELLHIP_SPACE_ELL;
    if (r->who == OPT_DEFAULT_ONLY) return option_refuse(*r, "this option is a creation-time default only (ellhip_set_default_option)");
    if (r->who == OPT_ELL && !ell) return option_refuse(*r, "this option exists on Ell only");
    if (r->who == OPT_STABLE && ell) return option_refuse(*r, "this option exists on EllStable only");
    long long* slot = option_slot(s, *r);  // (never NULL here: the read-only rows allow no value)
    if (r->first == FIRST_Q_CURRENT) {
        if (s->in_two_phase) return fail(ELLHIP_E_STATE, "update_begin without update_end");
        rc = make_q_current(s);
        if (rc) return rc;
        *slot = value;
        return option_schedule_changed(s);
    }
    if (r->first == FIRST_LEAVE_MIRROR) {
        rc = stable_mirror_leave(s);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    *slot = value;
    return 0;
}

int ellhip_get_option(const ellhip_space* s, int key, int64_t* value) {
    if (!s || !value) return fail(ELLHIP_E_INVALID, "NULL argument");
    switch (key) {  // read only or derived: not a stored value
        case ELLHIP_OPT_RESIDENT_ABANDONED: *value = s->rs_abandoned; return 0;
        case ELLHIP_OPT_STABLE_MIRRORED: *value = s->st_mirrored ? 1 : 0; return 0;
        case ELLHIP_OPT_STAGE_DIRECT: *value = s->stage_direct ? 1 : 0; return 0;
        case ELLHIP_OPT_PAD: *value = s->ld - s->n; return 0;
    }
    const OptionRow* r = option_row(key);
    const long long* slot = r ? option_slot(const_cast<ellhip_space*>(s), *r) : nullptr;
    if (!slot) return fail(ELLHIP_E_INVALID, "not a per-handle option");
    *value = *slot;
    return 0;
}

