"""GPU: every update schedule at the edges of the input range the reference handles (test_numeric_edges_cpu.py pins what
the oracle does there):
  * a power-of-two rescaled run (2^e g, 2^e beta), e = -200 / +200, is the same run: statuses, Q, xc and kappa to the bit,
    tsq exactly 4^e times as large -- a hidden absolute constant, a flushed subnormal or an overflowing association breaks it;
  * a zero gradient (omega = 0) inside every schedule -- in a matrix-core group, before an apply pass, in a resident batch,
    as the last recorded update of a depth-24 handle -- with both outcomes: Success (the state becomes NaN) and NoSoln (a
    queue halts, the state is the one before it);
  * a subnormal omega (|g| = 1e-154): finite where the oracle is finite;
  * a DIAGONALLY rescaled run -- start (D Q0 D, D xc0), cuts (D^-1 g, beta), D = diag(2^e_i), |e_i| <= 20 -- is the same run
    element by element: statuses, tsq and kappa to the bit, xc' = D xc and Q' = D Q D to the bit, on every single-handle Ell
    schedule (a sum that mixes elements of different rows or columns, or a stale element read, breaks it);
  * the host staging path (ELLHIP_OPT_STAGE_DIRECT = 0: k_stage pulls each gradient from pinned memory) against the direct
    write, with the caller's gradient buffer overwritten as soon as each call returns.
Each schedule is pinned by options (and the depth) on its handle, and profile_read() shows that its kernel class ran."""
from collections import namedtuple

import numpy as np
import pytest

from numeric_edges import (SCALE_EXPONENTS, assert_state_with_nans, beta, dense_start, diag_exponents, diag_scaled, mixed_seq,
                           oracle_run, queue_seq, scaled, state, subnormal_seq, with_zero)
from util import TOL, set_default

pytestmark = pytest.mark.gpu

Sched = namedtuple("Sched", "variant drive defaults depth opts")
LOW = {"SYMV_MIN_N": 512, "RESIDENT": 0}          # the lower-triangle (recorded, symmetric GEMV) schedule from n = 512 up
SCHEDULES = {
    "d1": Sched("ell", "direct", {}, 1, {}),                                      # ellhip_update, Q shrunk at every cut
    "rec8": Sched("ell", "direct", {}, 8, {}),                                    # n = 4096: recorded, full-row GEMV
    "low8-k1": Sched("ell", "direct", LOW, 8, {"APPLY_KERNEL": 1}),
    "low8-k2": Sched("ell", "direct", LOW, 8, {"APPLY_KERNEL": 2}),
    "low16-k1": Sched("ell", "direct", LOW, 16, {"APPLY_KERNEL": 1}),
    "low16-k2": Sched("ell", "direct", LOW, 16, {"APPLY_KERNEL": 2}),
    "low24-k1": Sched("ell", "direct", LOW, 24, {"APPLY_KERNEL": 1}),
    "low24-k2": Sched("ell", "direct", LOW, 24, {"APPLY_KERNEL": 2}),
    "pcc": Sched("ell", "pcc", {}, 1, {}),                                        # prime / cut / commit(next)
    "twophase": Sched("ell", "twophase", {}, 24, {}),                             # update_begin / update_end, n = 5120
    "q2p": Sched("ell", "queue", {"RESIDENT": 0}, 1, {}),                        # ellhip_queue_run: GEMV pass + rank-1 pass
    "qvalu": Sched("ell", "fused", LOW, 24, {"LOOKAHEAD": 3}),                   # groups of 3 on the vector ALU
    "qmfma": Sched("ell", "fused", LOW, 24, {"LOOKAHEAD": 32, "QUEUE_DEPTH": 48}),  # k_symm_mfma_q*, group stage, k_apply_mfma
    "res": Sched("ell", "fused", {"RESIDENT": 1}, None, {}),                      # the resident batch
    "st0": Sched("stable", "direct", {}, None, {"STABLE_SOLVE": 0}),
    "st0q": Sched("stable", "queue", {}, None, {"STABLE_SOLVE": 0}),
    "st3": Sched("stable", "direct", {}, None, {"STABLE_SOLVE": 3}),              # the mirrored layout
    "st3q": Sched("stable", "queue", {}, None, {"STABLE_SOLVE": 3}),
    "batch": Sched("batch", "batch", {}, None, {}),                               # EllBatch, B members
}
B = 4   # members of an EllBatch


def make(gpu, sid, n, start=None):
    """A handle pinned to schedule `sid`, profiling on.  start = (Q0, xc0): an Ell from that matrix and centre (kappa0 = 1)."""
    sp = SCHEDULES[sid]
    for k, v in sp.defaults.items():
        set_default(k, v)
    if sp.variant == "batch":
        return gpu.EllBatch.new_with_scalar(1.0, np.zeros((B, n)))
    if start is not None:
        assert sp.variant == "ell"
        e = gpu.Ell.new_with_matrix(1.0, start[0], start[1])
    else:
        e = (gpu.EllStable if sp.variant == "stable" else gpu.Ell).new_with_scalar(1.0, np.zeros(n))
    if sp.depth is not None:
        e.defer_depth = sp.depth
        assert e.defer_depth == sp.depth
    for k, v in sp.opts.items():
        e.set_option(getattr(gpu.capi, "OPT_" + k), v)
        assert e.get_option(getattr(gpu.capi, "OPT_" + k)) == v, (sid, k)
    if sid == "rec8":
        assert n < e.get_option(gpu.capi.OPT_SYMV_MIN_N)          # the full-row GEMV
    e.profile_enable(True)
    return e


def drive(gpu, e, sid, cuts, buf=None):
    """Statuses and tsq of every cut.  buf: every gradient goes in through this one array, which is overwritten with NaN
    as soon as the call that took it returns (the C ABI reads no caller memory after a call has returned)."""
    mode = SCHEDULES[sid].drive
    kinds, grads, b0, b1 = cuts
    k = len(kinds)
    if mode in ("queue", "fused"):
        e.queue_upload(kinds, grads, b0, b1)
        e.queue_run(0, k, fused=mode == "fused")
        return e.queue_results()

    def feed(i):
        if buf is None:
            return grads[i]
        buf[:] = grads[i]
        return buf

    def spoil():
        if buf is not None:
            buf[:] = np.nan

    st = np.empty(k, dtype=np.int32)
    ts = np.empty(k)
    if mode == "pcc":
        e.prime(feed(0))
        spoil()
    for i in range(k):
        if mode == "direct":
            st[i] = int(e._update(int(kinds[i]), (feed(i), beta(b0, b1, i))))
        elif mode == "pcc":
            st[i] = int(e.cut(int(kinds[i]), beta(b0, b1, i)))
            ts[i] = e.tsq()
            e.commit(feed(i + 1) if i + 1 < k else None)
        else:   # two-phase: begin (asynchronous GEMV) / end
            c0, c1 = beta(b0, b1, i)
            g = feed(i)
            gpu.capi.check(e._lib.ellhip_update_begin(e._h, int(kinds[i]), g.ctypes.data, c0, int(c1 is not None),
                                                      0.0 if c1 is None else c1), "ellhip_update_begin")
            spoil()
            st[i] = gpu.capi.check(e._lib.ellhip_update_end(e._h), "ellhip_update_end")
        spoil()
        if mode != "pcc":
            ts[i] = e.tsq()
    return st, ts


def run(gpu, sid, n, cuts, buf=None, start=None):
    """(statuses, tsq, (Q, xc, kappa), kernel launch counts) of one run on a fresh handle."""
    e = make(gpu, sid, n, start)
    st, ts = drive(gpu, e, sid, cuts, buf)
    if SCHEDULES[sid].variant == "stable" and st[st != 3][-1] == 0:
        # (the layout holds after a successful cut until an observer rebuilds the reference's buffer; a failed cut rewrites
        # the scratch triangle, src/ell_stable.rs:66, and leaves the handle in the reference's layout)
        assert e.get_option(gpu.capi.OPT_STABLE_MIRRORED) == (1 if sid.startswith("st3") else 0)
    s = state(e)                                                   # (observing Q applies what is still recorded)
    prof = {c: cnt for c, (_, cnt) in e.profile_read().items()}
    return st, ts, s, prof


def check_profile(sid, p, k):
    """The kernel class that defines the schedule ran (k: cuts that reached the engine)."""
    if sid in ("d1",):
        assert p["rank1"] > 0 and p["apply"] + p["apply_gemv"] + p["symv"] + p["resident"] == 0, p
    elif sid == "rec8":
        assert p["apply"] + p["apply_gemv"] > 0 and p["symv"] == 0, p
    elif sid.startswith("low") or sid == "twophase":
        assert p["symv"] > 0 and p["apply"] > 0, p
    elif sid == "pcc":
        assert p["fused"] > 0, p
    elif sid == "q2p":
        assert p["rank1"] > 0 and p["fused"] + p["resident"] + p["symv"] == 0, p
    elif sid == "qvalu":
        assert p["symv"] >= k // 3 and p["resident"] == 0, p              # groups of at most 3
    elif sid == "qmfma":
        assert 0 < p["symv"] <= max(1, k // 8) and p["resident"] == 0, p  # groups of up to 32 on the matrix cores
    elif sid == "res":
        assert p["resident"] >= 1 and p["rank1"] + p["symv"] == 0, p
    elif sid.startswith("st"):
        assert p["stable_fwd"] > 0 and p["stable_bwd"] > 0, p


# ---- sequences -------------------------------------------------------------------------------------------------------------

def _direct_k(sid):
    return 56 if sid.startswith(("low", "rec")) else 40


def sequence(orc, sid, n, seed, start=None):
    sp = SCHEDULES[sid]
    if sp.drive in ("queue", "fused"):
        return queue_seq(n, 24 if sid in ("res", "st0q", "st3q") else 56, seed)
    return mixed_seq(orc, n, _direct_k(sid), seed, stable=sp.variant == "stable", start=start)


def oracle_for(orc, sid, n, start=None):
    if start is not None:
        return orc.OracleEll.new_with_matrix(1.0, start[0], start[1])
    return (orc.OracleEllStable if SCHEDULES[sid].variant == "stable" else orc.OracleEll).new_with_scalar(1.0, np.zeros(n))


def check_against_oracle(orc, sid, n, cuts, st, ts, s, tol=TOL, start=None):
    halt = SCHEDULES[sid].drive in ("queue", "fused")
    o = oracle_for(orc, sid, n, start)
    ost, ots = oracle_run(o, cuts, halt=halt)
    assert np.array_equal(st, ost), (sid, list(st), list(ost))
    last = int(np.argmax(ost != 0)) if halt and np.any(ost != 0) else len(ost) - 1
    a, b = np.asarray(ts[:last + 1]), ots[:last + 1]
    assert np.array_equal(np.isnan(a), np.isnan(b)), (sid, "tsq NaN mask")
    fin = ~np.isnan(b)
    assert np.all(np.abs(a[fin] - b[fin]) <= tol * np.abs(b[fin]) + 1e-300), (sid, "tsq")
    assert_state_with_nans(s, state(o), tol, what=sid)
    return ost


def batch_run(gpu, n, member_cuts):
    """K cuts on each of the B members of one EllBatch (member b takes member_cuts[b]) -> statuses, tsq [K][B], per-member
    states."""
    e = make(gpu, "batch", n)
    kinds = np.stack([c[0] for c in member_cuts], axis=1)
    grads = np.stack([c[1] for c in member_cuts], axis=1)
    b0 = np.stack([c[2] for c in member_cuts], axis=1)
    b1 = np.stack([c[3] for c in member_cuts], axis=1)
    st, ts = e.update(kinds, grads, b0, b1)
    mq, xc, kap = e.mq, e.xc(), e.kappa
    return st, ts, [(mq[b], xc[b], float(kap[b])) for b in range(B)]


def assert_batch_is_the_oracle(orc, n, member_cuts, st, ts, states):
    """The batched engine follows the reference's statement order: every member bit for bit (NaN where the oracle has NaN)."""
    for b in range(B):
        o = orc.OracleEll.new_with_scalar(1.0, np.zeros(n))
        ost, ots = oracle_run(o, member_cuts[b])
        np.testing.assert_array_equal(st[:, b], ost)
        np.testing.assert_array_equal(ts[:, b], ots)
        for a, w in zip(states[b], state(o)):
            np.testing.assert_array_equal(a, w)


# ---- 1. rescaled runs are the same run ------------------------------------------------------------------------------------

RESCALE_CASES = [("d1", 64), ("d1", 1000), ("rec8", 4096), ("low8-k1", 1024), ("low8-k2", 1024), ("low16-k1", 1024),
                 ("low16-k2", 1024), ("low24-k1", 1024), ("low24-k2", 1024), ("pcc", 1000), ("q2p", 1000), ("qvalu", 1024),
                 ("qmfma", 1024), ("qmfma", 5120), ("res", 1000), ("res", 2048), ("res", 4096), ("st0", 640), ("st0q", 640),
                 ("st3", 640), ("st3q", 640)]


@pytest.mark.parametrize("sid,n", RESCALE_CASES, ids=[f"{s}-{n}" for s, n in RESCALE_CASES])
def test_rescaled_run_is_the_same_run(gpu, orc, sid, n):
    cuts = sequence(orc, sid, n, seed=7 * n + len(sid))
    st, ts, s, prof = run(gpu, sid, n, cuts)
    check_profile(sid, prof, len(cuts[0]))
    check_against_oracle(orc, sid, n, cuts, st, ts, s)
    for e in SCALE_EXPONENTS:
        st2, ts2, s2, _ = run(gpu, sid, n, scaled(cuts, e))
        assert np.array_equal(st2, st), (sid, e)
        assert np.array_equal(ts2, ts * 4.0 ** e), (sid, e, np.max(np.abs(ts2 / (ts * 4.0 ** e) - 1.0)))
        for name, a, b in zip(("Q", "xc", "kappa"), s2, s):
            assert np.array_equal(a, b), (sid, e, name, np.max(np.abs(np.asarray(a) - np.asarray(b))))


# the single-handle Ell schedules of RESCALE_CASES (EllStable and the batch engines: their packed layouts need an argument of
# their own)
DIAG_CASES = [(s, n) for s, n in RESCALE_CASES if SCHEDULES[s].variant == "ell" and (s, n) not in (("qmfma", 5120), ("res", 4096))]


@pytest.mark.parametrize("sid,n", DIAG_CASES, ids=[f"{s}-{n}" for s, n in DIAG_CASES])
def test_diagonally_rescaled_run_is_the_same_run(gpu, orc, sid, n):
    """Q -> D Q D, xc -> D xc, g -> D^-1 g with D = diag(2^e_i), |e_i| <= 20, betas unchanged: every product and every sum of
    the update scales by one power of two per element, so statuses, tsq and kappa keep their bits, xc' = D xc and Q' = D Q D bit
    for bit (tests/test_numeric_edges_cpu.py pins it on the oracle).  Both runs start through new_with_matrix from
    util.dense_spd and a non-zero centre; the unscaled one is checked against the oracle."""
    seed = 9 * n + len(sid)
    start = dense_start(n, seed)
    cuts = sequence(orc, sid, n, seed=seed + 2, start=start)
    st, ts, s, prof = run(gpu, sid, n, cuts, start=start)
    check_profile(sid, prof, len(cuts[0]))
    check_against_oracle(orc, sid, n, cuts, st, ts, s, start=start)
    e = diag_exponents(n, seed + 3)
    d = np.ldexp(1.0, e)
    st2, ts2, (q2, xc2, kappa2), prof2 = run(gpu, sid, n, diag_scaled(cuts, e), start=dense_start(n, seed, e))
    check_profile(sid, prof2, len(cuts[0]))
    assert np.array_equal(st2, st), (sid, list(st2), list(st))
    assert np.array_equal(ts2, ts), (sid, "tsq", np.max(np.abs(ts2 / ts - 1.0)))
    assert kappa2 == s[2], (sid, "kappa", kappa2, s[2])
    assert np.array_equal(xc2, d * s[1]), (sid, "xc", int(np.sum(xc2 != d * s[1])))
    want = d[:, None] * s[0] * d[None, :]
    bad = np.argwhere(q2 != want)
    assert bad.size == 0, (sid, "Q", len(bad), bad[:4].tolist(), float(np.max(np.abs(q2 / want - 1.0))))


@pytest.mark.parametrize("n", [16, 128])
def test_rescaled_batch_is_the_same_run(gpu, orc, n):
    member_cuts = [mixed_seq(orc, n, 24, 300 + 7 * b + n) for b in range(B)]
    st, ts, states = batch_run(gpu, n, member_cuts)
    assert_batch_is_the_oracle(orc, n, member_cuts, st, ts, states)
    for e in SCALE_EXPONENTS:
        st2, ts2, states2 = batch_run(gpu, n, [scaled(c, e) for c in member_cuts])
        assert np.array_equal(st2, st) and np.array_equal(ts2, ts * 4.0 ** e), e
        for b in range(B):
            for a, w in zip(states2[b], states[b]):
                assert np.array_equal(a, w), (e, b)


def test_rescaled_run_at_full_size(gpu):
    """n = 16384 in the default configuration (depth 24, groups of up to 32 on the matrix cores, the rank-48 apply pass): 60
    parallel cuts from synth, rescaled by 2^-200, give the same bits.  No oracle: the relation itself is the check."""
    from ellalgo_rs_amd import synth
    n, k, ex = 16384, 60, -200
    cuts = synth.parallel_cuts(n, k)
    outs = []
    for c in (cuts, scaled(tuple(np.asarray(a) for a in cuts), ex)):
        e = gpu.Ell.new_with_scalar(1.0, np.zeros(n))
        assert e.defer_depth == 24 and e.get_option(gpu.capi.OPT_LOOKAHEAD) == 32
        e.profile_enable(True)
        e.queue_upload(*c)
        e.queue_run(0, k, fused=True)
        st, ts = e.queue_results()
        assert np.all(st == 0)
        assert 0 < e.profile_read()["symv"][1] <= k // 8
        outs.append((ts, e.xc(), e.kappa, e.mq))
        del e
    (ta, xa, ka, qa), (tb, xb, kb, qb) = outs
    assert np.array_equal(tb, ta * 4.0 ** ex) and np.array_equal(xa, xb) and ka == kb
    for r in range(0, n, 1024):
        assert np.array_equal(qa[r:r + 1024], qb[r:r + 1024]), f"rows {r}.."


# ---- 2. a zero gradient inside every schedule ------------------------------------------------------------------------------

ZERO_CASES = [("qmfma", 1024, 0), ("qmfma", 1024, 5), ("qmfma", 1024, 17),     # first / second 16-wide column tile of a group
              ("qmfma", 1024, 47),                                             # the last cut before the rank-48 apply pass
              ("res", 2048, 0), ("res", 2048, 11),                             # first and a middle cut of a resident batch
              ("low24-k2", 1024, 23), ("low24-k1", 1024, 23),                  # the 24th recorded update
              ("low8-k1", 1024, 7), ("low16-k2", 1024, 15), ("rec8", 4096, 7),  # the last cut before an apply pass
              ("d1", 64, 5), ("pcc", 1000, 5), ("q2p", 1000, 5), ("qvalu", 1024, 5),
              ("st0", 64, 5), ("st3", 640, 5), ("st3q", 640, 5)]


@pytest.mark.parametrize("outcome", ["nan", "nosoln"])
@pytest.mark.parametrize("sid,n,pos", ZERO_CASES, ids=[f"{s}-{n}-at{p}" for s, n, p in ZERO_CASES])
def test_zero_gradient_inside_the_schedule(gpu, orc, sid, n, pos, outcome):
    """Success (bias cut, beta = 0: tsq = 0, xc / Q / kappa NaN, every later cut Success with tsq NaN) or NoSoln (beta > 0: a
    queue halts there with tsq = 0 and the state before it): statuses exactly, NaN masks of tsq, xc, kappa and Q (EllStable:
    the packed buffer) equal to the oracle's, finite entries to the north-star tolerance."""
    queued = SCHEDULES[sid].drive in ("queue", "fused")
    # the queue sequence has no failing cut of its own, so cut `pos` is the (pos + 1)-th recorded update
    cuts = queue_seq(n, (24 if sid in ("res", "st3q") else 56) if queued else pos + 6, seed=11 * n + pos)
    k = len(cuts[0])
    assert k >= pos + 3
    cuts = with_zero(cuts, [pos], outcome)
    st, ts, s, _ = run(gpu, sid, n, cuts)
    ost = check_against_oracle(orc, sid, n, cuts, st, ts, s)
    assert ost[pos] == (0 if outcome == "nan" else 1) and ts[pos] == 0.0
    if outcome == "nan":
        assert np.isnan(s[1]).all() and np.isnan(s[2])


@pytest.mark.parametrize("sid,n", [("d1", 64), ("qmfma", 1024), ("res", 2048), ("st3", 640)])
def test_zero_gradient_central_cut(gpu, orc, sid, n):
    """A central cut on a zero gradient: Success with tsq = 0; kappa stays finite (the central cut does not see omega), xc
    and Q turn NaN."""
    cuts = queue_seq(n, 24 if SCHEDULES[sid].drive in ("queue", "fused") else 12, seed=13 * n)
    cuts = with_zero(cuts, [5], "central")
    st, ts, s, _ = run(gpu, sid, n, cuts)
    ost = check_against_oracle(orc, sid, n, cuts, st, ts, s)
    assert ost[5] == 0 and ts[5] == 0.0


@pytest.mark.parametrize("n", [16, 128])
def test_zero_gradient_in_one_batch_member(gpu, orc, n):
    """Member 1 turns NaN at cut 3, member 2 meets a NoSoln zero cut at cut 5: every member -- the healthy ones above all --
    stays bit-identical to its own oracle run."""
    member_cuts = [mixed_seq(orc, n, 12, 500 + 7 * b + n) for b in range(B)]
    member_cuts[1] = with_zero(member_cuts[1], [3], "nan")
    member_cuts[2] = with_zero(member_cuts[2], [5], "nosoln")
    st, ts, states = batch_run(gpu, n, member_cuts)
    assert_batch_is_the_oracle(orc, n, member_cuts, st, ts, states)
    assert np.isnan(states[1][1]).all() and np.isfinite(states[0][0]).all() and np.isfinite(states[3][0]).all()


# ---- 3. subnormal omega ----------------------------------------------------------------------------------------------------

SUBNORMAL_CASES = [("d1", 64), ("d1", 1000), ("low24-k2", 1024), ("qmfma", 1024), ("res", 2048), ("st3", 640)]


@pytest.mark.parametrize("sid,n", SUBNORMAL_CASES, ids=[f"{s}-{n}" for s, n in SUBNORMAL_CASES])
def test_subnormal_omega(gpu, orc, sid, n):
    """Eight central cuts with |g| = 1e-154 from Q0 = I: omega ~ 1e-308 is subnormal, its terms g_i gt_i ~ 1e-308 / n more so.
    Each product rounds to the subnormal quantum q = 2^-1074 (absolute), so omega carries up to n q / 2 of absolute error
    per engine whatever the summation order -- a relative n q / omega, which at n = 1024 is 5e-13.  That error enters tsq,
    xc (through rho / omega) and Q (through sigma / omega) about one to one and adds up over the K cuts: the tolerance is
    4 K n q / min omega (1.6e-11 at n = 1024), plus 1e-14 for the ordinary rounding of two summation orders; it must stay
    below 1e-8.  A path that flushes subnormals to zero gets omega = 0 and a NaN state, or omega off by its lost terms."""
    cuts = subnormal_seq(n)
    k = len(cuts[0])
    o = oracle_for(orc, sid, n)
    _, ots = oracle_run(o, cuts)
    tol = 4.0 * k * n * 2.0 ** -1074 / float(np.min(ots)) + 1e-14
    assert tol <= 1e-8
    st, ts, s, prof = run(gpu, sid, n, cuts)
    check_profile(sid, prof, k)
    check_against_oracle(orc, sid, n, cuts, st, ts, s, tol=tol)
    assert np.all(np.isfinite(s[0])) and np.all(np.isfinite(s[1]))


@pytest.mark.parametrize("n", [16, 128])
def test_subnormal_omega_batch(gpu, orc, n):
    member_cuts = [subnormal_seq(n, seed=40 + b) for b in range(B)]
    st, ts, states = batch_run(gpu, n, member_cuts)
    assert_batch_is_the_oracle(orc, n, member_cuts, st, ts, states)
    assert all(np.isfinite(x[0]).all() for x in states)


# ---- 4. the host staging path ----------------------------------------------------------------------------------------------

STAGE_CASES = [("d1", 1000), ("rec8", 4096), ("pcc", 1000), ("twophase", 5120), ("st3", 640)]


@pytest.mark.parametrize("sid,n", STAGE_CASES, ids=[f"{s}-{n}" for s, n in STAGE_CASES])
def test_staging_path_equals_the_direct_write(gpu, orc, sid, n):
    """STAGE_DIRECT = 0 (gradients pass through a pinned host slot and k_stage) and = 1 (where the device has a large BAR: the
    host writes the device slot itself) stage the same bytes, so the runs agree to the bit; both are fed from ONE buffer
    the test overwrites with NaN right after each call returns, and the first one is checked against the oracle."""
    cuts = mixed_seq(orc, n, 30 if sid == "twophase" else 40, seed=5 * n + len(sid))
    outs = []
    for direct in (0, 1):
        set_default("STAGE_DIRECT", direct)
        e = make(gpu, sid, n)
        if direct == 0:
            assert e.get_option(gpu.capi.OPT_STAGE_DIRECT) == 0
        buf = np.empty(n)
        st, ts = drive(gpu, e, sid, cuts, buf)
        s = state(e)
        check_profile(sid, {c: cnt for c, (_, cnt) in e.profile_read().items()}, len(st))
        outs.append((st, ts, s))
        del e
    (sa, ta, xa), (sb, tb, xb) = outs
    assert np.array_equal(sa, sb) and np.array_equal(ta, tb)
    for name, a, b in zip(("Q", "xc", "kappa"), xa, xb):
        assert np.array_equal(a, b), name
    check_against_oracle(orc, sid, n, cuts, sa, ta, xa)
