"""GPU: the batched device-resident low-pass design loop on a streamed batch handle
(include/ellhip_batch_lowpass_streamed.h) against the CPU oracle (oracle.OracleLowpass over OracleEll, through
tests/batch_lowpass_reference.py) and against the same loop on the LDS engine.  The kernel follows the reference's statement
order, so every comparison is EXACT: == on float64 bits and on integers -- niter, status, has_best, gamma, x_best, the
oracle state (cursors, kmax, fmax, more_alt, sp_sq) and the spaces' Q, xc, kappa and tsq afterwards.

The pinned counts are those of tests/test_batch_lowpass_streamed_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import batch_lowpass_reference as ref
from lowpass_probes import CONSTANT_SETS, probe_points

pytestmark = pytest.mark.gpu

MAX_ITERS, TOL = ref.MAX_ITERS, ref.TOL


def same_bits(a, b, what=""):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na = np.isnan(a)
    np.testing.assert_array_equal(na, np.isnan(b), err_msg=what + ": NaN positions")
    np.testing.assert_array_equal(a[~na].view(np.uint64), b[~na].view(np.uint64), err_msg=what + ": bits")


def new_spaces(gpu, B, n):
    batch = gpu.EllBatchStreamed.new_with_scalar(np.full(B, ref.KAPPA), np.zeros((B, n)))
    assert batch.is_streamed
    return batch


def make_gpu(gpu, n, consts_list, chunk=None):
    prob = gpu.BatchLowpassProblem.streamed(n, *ref.columns(consts_list))
    if chunk is not None:
        prob.set_chunk(chunk)
    return prob, new_spaces(gpu, len(consts_list), n)


def assert_state_equal(prob, states, what=""):
    got, want = prob.state(), ref.stack_state(states)
    for k in ref.STATE_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    same_bits(got["fmax"], want["fmax"], what + " fmax")
    same_bits(got["sp_sq"], want["sp_sq"], what + " sp_sq")


def assert_spaces_equal(batch, recs):
    same_bits(batch.mq, np.stack([np.array(r["mq"]) for r in recs]), "mq")
    same_bits(batch.xc(), np.stack([np.array(r["xc"]) for r in recs]), "xc")
    same_bits(batch.kappa, np.array([r["kappa"] for r in recs]), "kappa")
    same_bits(batch.tsq(), np.array([r["tsq"] for r in recs]), "tsq")


def assert_runs_equal(got, recs, n):
    x_best, has, niter, gamma, status = got
    np.testing.assert_array_equal(niter, np.array([r["niter"] for r in recs], dtype=np.int64))
    np.testing.assert_array_equal(status, np.array([r["status"] for r in recs], dtype=np.int32))
    np.testing.assert_array_equal(has, np.array([r["x_best"] is not None for r in recs], dtype=np.int32))
    if gamma is not None:
        same_bits(gamma, np.array([r["gamma"] for r in recs]), "gamma")
    want = np.stack([np.full(n, np.nan) if r["x_best"] is None else r["x_best"] for r in recs])
    same_bits(x_best, want, "x_best")  # rows without a result stay as the caller left them (NaN)


def assert_all_equal(prob, batch, got, recs, n):
    assert_runs_equal(got, recs, n)
    assert_state_equal(prob, [r["state"] for r in recs])
    assert_spaces_equal(batch, recs)


def run_optim(prob, batch, consts_list, max_iters=MAX_ITERS, tol=TOL):
    return prob.optim(batch, np.array([c[4] for c in consts_list]), max_iters, tol)


def check_optim(gpu, n, consts_list, max_iters=MAX_ITERS, tol=TOL, chunk=None):
    recs = [ref.solve_optim(n, tuple(c), max_iters, tol) for c in consts_list]
    prob, batch = make_gpu(gpu, n, consts_list, chunk)
    assert_all_equal(prob, batch, run_optim(prob, batch, consts_list, max_iters, tol), recs, n)
    return recs


def check_feas(gpu, n, consts_list, max_iters=MAX_ITERS, tol=TOL):
    recs = [ref.solve_feas(n, tuple(c), max_iters, tol) for c in consts_list]
    prob, batch = make_gpu(gpu, n, consts_list)
    x, ok, niter, status = prob.feas(batch, max_iters, tol)
    assert_all_equal(prob, batch, (x, ok, niter, None, status), recs, n)
    return recs


# ---- 1. complete runs against the CPU ---------------------------------------------------------------------------------------
PINS = [
    (129, ref.LOOSE, 2252, ref.NOSOLN, True, 148, True),
    (130, ref.SHORT_PASSBAND, 2246, ref.NOSOLN, True, 142, True),
    (130, ref.EMPTY_TRANSITION, 337, ref.NOSOLN, False, 337, False),
    (129, ref.NO_STOPBAND_B, 212, ref.UNKNOWN, False, 212, True),   # Unknown: niter not advanced by the last round
    (129, ref.NO_STOPBAND_A, 177, ref.UNKNOWN, False, 177, True),
    (130, ref.FEAS_INFEASIBLE, 846, ref.NOSOLN, True, 300, True),
    (191, ref.CORRECTED, 2641, ref.NOSOLN, True, 284, True),
    (200, ref.family(1), 3193, ref.NOSOLN, True, 250, True),
    (256, ref.LOOSE, 4275, ref.NOSOLN, True, 300, True),
]


@pytest.mark.parametrize("n,consts,niter,status,best,fniter,feasible", PINS, ids=[f"{p[0]}-{p[1][0]}-{p[1][1]}" for p in PINS])
def test_complete_runs(gpu, n, consts, niter, status, best, fniter, feasible):
    r = check_optim(gpu, n, [consts] * 2)[0]
    assert (r["niter"], r["status"], r["x_best"] is not None) == (niter, status, best)
    f = check_feas(gpu, n, [consts] * 2)[0]
    assert (f["niter"], f["x_best"] is not None) == (fniter, feasible)


def test_mixed_batch_stops_at_different_iterations(gpu):
    consts = [ref.family(s) for s in range(6)] + [ref.NO_STOPBAND_B, ref.EMPTY_TRANSITION]
    recs = check_optim(gpu, 136, consts)
    assert recs[6]["status"] == ref.UNKNOWN and recs[6]["niter"] < min(r["niter"] for r in recs[:6])
    assert len({r["niter"] for r in recs}) > 4
    check_feas(gpu, 136, consts)


# ---- 2. large blocks, cut off by max_iters ----------------------------------------------------------------------------------
def test_n512(gpu):
    r = check_optim(gpu, 512, [ref.LOOSE], max_iters=700)[0]
    assert r["niter"] == 700 and r["x_best"] is not None and r["gamma"] == 0.1536537185113417
    f = check_feas(gpu, 512, [ref.LOOSE])[0]
    assert f["niter"] == 608 and f["x_best"] is not None


CONSTS_1024 = [ref.LOOSE, ref.family(0)]


@pytest.fixture(scope="module")
def prob1024(gpu):
    """the n = 1024 table is 240 MiB: one handle for the module"""
    prob = gpu.BatchLowpassProblem.streamed(1024, *ref.columns(CONSTS_1024))
    yield prob
    del prob


def as_new(prob, consts_list):
    """The shared handle as its constructor left it, whatever ran before: assess_optim sets sp_sq to the gamma it is given
    (src/oracles/lowpass_oracle.rs:140), reset() restores the cursors, fmax and kmax."""
    prob.assess_optim(np.zeros((prob.B, prob.n)), np.array([c[4] for c in consts_list]))
    prob.reset()
    prob.set_chunk(256)


def test_n1024_optim_and_feas(gpu, prob1024):
    n = 1024
    as_new(prob1024, CONSTS_1024)
    recs = [ref.solve_optim(n, c, 150, TOL) for c in CONSTS_1024]
    assert all(r["niter"] == 150 and r["x_best"] is None for r in recs)
    batch = new_spaces(gpu, 2, n)
    assert_all_equal(prob1024, batch, run_optim(prob1024, batch, CONSTS_1024, 150), recs, n)
    as_new(prob1024, CONSTS_1024)
    recs = [ref.solve_feas(n, c, 150, TOL) for c in CONSTS_1024]
    batch = new_spaces(gpu, 2, n)
    x, ok, niter, status = prob1024.feas(batch, 150, TOL)
    assert_all_equal(prob1024, batch, (x, ok, niter, None, status), recs, n)


@pytest.mark.parametrize("n,max_iters", [(1023, 60), (193, 300)])
def test_odd_n_in_a_padded_block(gpu, n, max_iters):
    r = check_optim(gpu, n, [ref.LOOSE, ref.family(2)], max_iters=max_iters)[0]
    assert r["niter"] == max_iters and r["status"] == ref.SUCCESS


# ---- 3. against the LDS engine ------------------------------------------------------------------------------------------------
def lds_and_streamed(gpu, n, consts):
    B = len(consts)
    cols = ref.columns(consts)
    lds = (gpu.BatchLowpassProblem(n, *cols), gpu.EllBatch.new_with_scalar(np.full(B, ref.KAPPA), np.zeros((B, n))))
    st = (gpu.BatchLowpassProblem.streamed(n, *cols), new_spaces(gpu, B, n))
    return lds, st


def assert_engines_equal(lds, st, got_l, got_s):
    for a, b, what in zip(got_l, got_s, ("x", "has", "niter", "gamma", "status")):
        if a is None:
            continue
        same_bits(a, b, what) if a.dtype == np.float64 else np.testing.assert_array_equal(a, b, err_msg=what)
    sl, ss = lds[0].state(), st[0].state()
    for k in ref.STATE_KEYS:
        same_bits(sl[k], ss[k], k) if sl[k].dtype == np.float64 else np.testing.assert_array_equal(sl[k], ss[k], err_msg=k)
    same_bits(lds[1].mq, st[1].mq, "mq")
    same_bits(lds[1].xc(), st[1].xc(), "xc")
    same_bits(lds[1].kappa, st[1].kappa, "kappa")
    same_bits(lds[1].tsq(), st[1].tsq(), "tsq")


@pytest.mark.parametrize("n", [1, 2, 16, 33, 64, 128])
def test_optim_equals_the_lds_engine(gpu, n):
    consts = [ref.LOOSE, ref.family(0), ref.family(4)]
    lds, st = lds_and_streamed(gpu, n, consts)
    got_l = run_optim(*lds, consts)
    got_s = run_optim(*st, consts)
    assert_engines_equal(lds, st, got_l, got_s)
    if n == 1:  # the state turns NaN and the oracle finds nothing to cut with
        assert (got_s[4] == ref.UNKNOWN).all() and np.isnan(st[1].mq).all()
    else:
        assert got_s[2].max() > 5


@pytest.mark.parametrize("n", [16, 128])
def test_feas_equals_the_lds_engine(gpu, n):
    consts = [ref.LOOSE, ref.FEAS_INFEASIBLE, ref.family(3)]
    lds, st = lds_and_streamed(gpu, n, consts)
    x_l, ok_l, niter_l, status_l = lds[0].feas(lds[1], MAX_ITERS, TOL)
    x_s, ok_s, niter_s, status_s = st[0].feas(st[1], MAX_ITERS, TOL)
    assert_engines_equal(lds, st, (x_l, ok_l, niter_l, None, status_l), (x_s, ok_s, niter_s, None, status_s))
    assert ok_s[0] == 1 and (niter_s > 5).all()


# ---- 4. fusion changes nothing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunking_changes_nothing(gpu, chunk):
    """chunk 1: no sweep is ever fused; chunk 7: six fused rounds, then a plain one; 256: all but every 256th fused"""
    check_optim(gpu, 129, [ref.LOOSE], chunk=chunk)


# ---- 5. stops and continuations ---------------------------------------------------------------------------------------------------
def test_max_iters_zero_moves_nothing(gpu):
    n, consts = 129, [ref.family(s) for s in range(3)]
    prob, batch = make_gpu(gpu, n, consts)
    before = (batch.mq, batch.xc(), batch.kappa, batch.tsq(), prob.state())
    x_best, has, niter, gamma, status = prob.optim(batch, 0.05, 0, TOL)
    assert (niter == 0).all() and (has == 0).all() and (status == ref.SUCCESS).all() and np.isnan(x_best).all()
    assert (gamma == 0.05).all()
    after = (batch.mq, batch.xc(), batch.kappa, batch.tsq(), prob.state())
    for a, b in zip(before[:4], after[:4]):
        same_bits(a, b)
    for k in ref.STATE_KEYS:
        np.testing.assert_array_equal(before[4][k], after[4][k])


def cpu_record(omega, space, out):
    xb, niter, gamma, status = out
    return dict(x_best=xb, niter=niter, gamma=gamma, status=status, state=omega.state(), **ref.space_record(space))


def test_cut_off_continue_and_reset(gpu):
    n, consts = 130, [ref.family(s) for s in range(3)]
    full = [ref.solve_optim(n, c) for c in consts]
    pairs = [ref.fresh(n, c) for c in consts]
    first = [cpu_record(o, s, o.cutting_plane_optim(s, c[4], 100, TOL)) for (o, s), c in zip(pairs, consts)]
    assert all(r["niter"] == 100 for r in first)
    prob, batch = make_gpu(gpu, n, consts)
    got = run_optim(prob, batch, consts, 100)
    assert_all_equal(prob, batch, got, first, n)
    second = [cpu_record(o, s, o.cutting_plane_optim(s, r["gamma"], MAX_ITERS - 100, TOL)) for (o, s), r in zip(pairs, first)]
    for r, f in zip(second, full):  # the CPU run driven this way is the uninterrupted run
        assert r["niter"] + 100 == f["niter"] and r["gamma"] == f["gamma"] and r["state"] == f["state"]
        assert np.array_equal(r["mq"], f["mq"])
    got2 = prob.optim(batch, got[3], MAX_ITERS - 100, TOL)
    assert_all_equal(prob, batch, got2, second, n)
    # reset: cursors, fmax and kmax as after new(); a rerun from fresh spaces reproduces the whole run
    prob.reset()
    s = prob.state()
    np.testing.assert_array_equal(s["idx1"], np.full(3, -1))
    np.testing.assert_array_equal(s["idx2"], s["nwpass"] - 1)
    np.testing.assert_array_equal(s["idx3"], s["nwstop"] - 1)
    assert (s["fmax"] == -np.inf).all() and (s["kmax"] == -1).all() and (s["more_alt"] == 1).all()
    batch = new_spaces(gpu, 3, n)
    assert_all_equal(prob, batch, run_optim(prob, batch, consts), full, n)


def test_batch_update_between_two_loops(gpu):
    n, B = 129, 4
    consts = [ref.family(s) for s in range(B)]
    prob, batch = make_gpu(gpu, n, consts)
    pairs = [ref.fresh(n, c) for c in consts]
    first = [cpu_record(o, s, o.cutting_plane_optim(s, c[4], 60, TOL)) for (o, s), c in zip(pairs, consts)]
    got = run_optim(prob, batch, consts, 60)
    assert_all_equal(prob, batch, got, first, n)
    rng = np.random.default_rng(3)
    grads = rng.standard_normal((1, B, n))
    kinds = rng.integers(0, 2, size=(1, B)).astype(np.int32)
    beta = np.zeros((1, B))
    want = np.zeros((1, B), dtype=np.int32)
    for b, (omega, space) in enumerate(pairs):
        beta[0, b] = 0.1 * np.sqrt(space.tsq) if kinds[0, b] == 0 else 0.0
        want[0, b] = space.update(int(kinds[0, b]), grads[0, b], beta[0, b])
    status, _ = batch.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    assert_spaces_equal(batch, [ref.space_record(space) for _, space in pairs])
    second = [cpu_record(o, s, o.cutting_plane_optim(s, r["gamma"], 400, TOL)) for (o, s), r in zip(pairs, first)]
    assert_all_equal(prob, batch, prob.optim(batch, got[3], 400, TOL), second, n)


def test_tolerance_stop_completes_the_last_update(gpu):
    """a tolerance taken from the CPU run's own tsq sequence: the first round from 50 on whose tsq is a new minimum"""
    n, consts = 129, ref.LOOSE
    omega, space = ref.fresh(n, consts)
    gamma, tsq = consts[4], []
    for _ in range(200):
        _, niter, gamma, status = omega.cutting_plane_optim(space, gamma, 1, 0.0)
        assert niter == 1 and status == ref.SUCCESS
        tsq.append(space.tsq)
    k = next(k for k in range(50, 200) if tsq[k] < min(tsq[:k]))
    tol = 0.5 * (tsq[k] + min(tsq[:k]))
    rec = check_optim(gpu, n, [consts] * 2, tol=tol)[0]
    assert rec["niter"] == k and rec["status"] == ref.SUCCESS and rec["tsq"] == tsq[k] < tol


# ---- 6. flags and starts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["no_defer_trick", "use_parallel_cut"])
def test_flags(gpu, flag):
    n, consts, iters = 129, [ref.LOOSE, ref.family(1)], 300
    prob, batch = make_gpu(gpu, n, consts)
    pairs = [ref.fresh(n, c) for c in consts]
    if flag == "no_defer_trick":
        batch.set_no_defer_trick(True)
    else:
        batch.set_use_parallel_cut(False)
    for _, space in pairs:
        space.set_no_defer_trick(True) if flag == "no_defer_trick" else space.set_use_parallel_cut(False)
    recs = [cpu_record(o, s, o.cutting_plane_optim(s, c[4], iters, TOL)) for (o, s), c in zip(pairs, consts)]
    plain = ref.solve_optim(n, consts[0], iters, TOL)
    assert not np.array_equal(recs[0]["mq"], plain["mq"])  # the flag does something
    assert_all_equal(prob, batch, run_optim(prob, batch, consts, iters), recs, n)


@pytest.mark.parametrize("n", [64, 129])
def test_non_symmetric_start(gpu, orc, n):
    """the first successful cut takes the two-phase path and mirrors the lower triangle; with no successful cut the
    caller's matrix comes back verbatim"""
    rng = np.random.default_rng(90 + n)
    consts = [ref.LOOSE, ref.family(2), ref.AS_WRITTEN]
    B = len(consts)
    kappa = np.full(B, ref.KAPPA)
    mq = np.stack([np.eye(n) * (1.0 + rng.random()) + (0.1 / n) * rng.standard_normal((n, n)) for _ in range(B)])
    prob = gpu.BatchLowpassProblem.streamed(n, *ref.columns(consts))
    batch = gpu.EllBatchStreamed.new_with_matrix(kappa, mq, np.zeros((B, n)))
    recs = []
    for b, c in enumerate(consts):
        omega = orc.OracleLowpass(n, *c)
        space = orc.OracleEll.new_with_matrix(kappa[b], mq[b], np.zeros(n))
        recs.append(cpu_record(omega, space, omega.cutting_plane_optim(space, c[4], 40, TOL)))
    assert recs[0]["niter"] == 40 and recs[2]["niter"] == 0 and recs[2]["status"] == ref.NOSOLN
    assert_all_equal(prob, batch, run_optim(prob, batch, consts, 40), recs, n)
    q = batch.mq
    same_bits(q[2], mq[2], "no successful cut: the caller's matrix verbatim")
    assert not np.array_equal(q[2], q[2].T)
    same_bits(q[:2], np.swapaxes(q[:2], 1, 2), "mirrored")


def test_from_space_clone(gpu):
    n, consts = 129, [ref.family(s) for s in range(3)]
    base = gpu.Ell.new_with_scalar(ref.KAPPA, np.zeros(n))
    batch = gpu.EllBatchStreamed.from_space(base, 3)
    assert batch.is_streamed
    prob = gpu.BatchLowpassProblem.streamed(n, *ref.columns(consts))
    recs = [ref.solve_optim(n, c, 200, TOL) for c in consts]
    assert_all_equal(prob, batch, run_optim(prob, batch, consts, 200), recs, n)


# ---- 7. more workgroups than CUs --------------------------------------------------------------------------------------------------
def test_large_population(gpu):
    three = [ref.LOOSE, ref.family(1), ref.family(5)]
    check_optim(gpu, 129, three * 200, max_iters=40)


# ---- 8. the oracle call by call -----------------------------------------------------------------------------------------------------
def compare_calls(prob, omegas, consts, n, seed):
    B = len(omegas)
    np.testing.assert_array_equal(prob.spectrum, omegas[0].spectrum)
    assert_state_equal(prob, [o.state() for o in omegas], "new")
    ncut = 0
    for it, x in enumerate(probe_points(n, np.random.default_rng(seed), 10)):
        want = [o.assess_feas(x) for o in omegas]
        grad, b0, has1, b1, cut = prob.assess_feas(np.tile(x, (B, 1)))
        for b, w in enumerate(want):
            assert cut[b] == (w is not None), (it, b)
            if w is None:
                assert np.isnan(grad[b]).all() and np.isnan(b0[b])  # untouched
                continue
            ncut += 1
            g, (w0, w1) = w
            same_bits(grad[b], g, f"call {it} instance {b}")
            assert b0[b] == w0 and has1[b] == (w1 is not None) and (w1 is None or b1[b] == w1), (it, b, b0[b], b1[b], w)
        assert_state_equal(prob, [o.state() for o in omegas], f"call {it}")
    assert ncut > 0
    gamma = np.array([c[4] for c in consts])
    for it, x in enumerate(probe_points(n, np.random.default_rng(seed + 1), 8)):
        grad, b0, has1, b1, shrunk, gamma_out, rc = prob.assess_optim(np.tile(x, (B, 1)), gamma)
        for b, o in enumerate(omegas):
            (g, (w0, w1)), sh, ga = o.assess_optim(x, gamma[b])
            assert rc[b] == 1 and shrunk[b] == sh and gamma_out[b] == ga, (it, b)
            same_bits(grad[b], g, f"optim call {it} instance {b}")
            assert b0[b] == w0 and has1[b] == (w1 is not None) and (w1 is None or b1[b] == w1), (it, b)
        assert_state_equal(prob, [o.state() for o in omegas], f"optim call {it}")
        gamma = gamma_out


@pytest.mark.parametrize("n", [129, 320])
def test_oracle_call_by_call(gpu, orc, n):
    consts = [tuple(CONSTANT_SETS[k]) for k in ("corrected", "loose", "very_loose", "negative_passband_allowed")]
    prob = gpu.BatchLowpassProblem.streamed(n, *ref.columns(consts))
    compare_calls(prob, [orc.OracleLowpass(n, *c) for c in consts], consts, n, 7 + n)


def test_oracle_call_by_call_n1024(gpu, orc, prob1024):
    as_new(prob1024, CONSTS_1024)
    compare_calls(prob1024, [orc.OracleLowpass(1024, *c) for c in CONSTS_1024], CONSTS_1024, 1024, 5)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_spaces_untouched(gpu):
    capi = gpu.capi
    lib = capi.load()
    n, B = 16, 3
    cols = ref.columns([ref.LOOSE] * B)
    prob = gpu.BatchLowpassProblem.streamed(n, *cols)
    rng = np.random.default_rng(2)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(batch, entry, problem=prob):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        gamma = np.full(batch.B, 0.3)
        xb = np.full((batch.B, batch.n), np.nan)
        has = np.zeros(batch.B, dtype=np.int32)
        niter = np.zeros(batch.B, dtype=np.int64)
        status = np.zeros(batch.B, dtype=np.int32)
        if "optim" in entry:
            rc = getattr(lib, entry)(batch._h, problem._h, ptr(gamma), 100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status))
        else:
            rc = getattr(lib, entry)(batch._h, problem._h, 100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status))
        assert rc == capi.E_INVALID and lib.ellhip_last_error()
        for a, b in zip(before, (batch.mq, batch.xc(), batch.kappa, batch.tsq())):
            same_bits(a, b, "untouched")
        assert np.isnan(xb).all()

    x0 = rng.standard_normal((B, n))
    for entry in ("ellhip_batch_lowpass_optim_streamed", "ellhip_batch_lowpass_feas_streamed"):
        refused(gpu.EllBatch.new_with_scalar(np.full(B, 10.0), x0), entry)            # an LDS handle
        refused(gpu.EllStableBatch.new_with_scalar(np.full(B, 10.0), x0), entry)
        refused(gpu.EllBatchStreamed.new_with_scalar(np.full(B + 1, 10.0), rng.standard_normal((B + 1, n))), entry)  # wrong B
        refused(gpu.EllBatchStreamed.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n + 1))), entry)      # wrong n
    h = C.c_void_p()
    for bad_n in (1025, 0):
        assert lib.ellhip_batch_lowpass_create_streamed(C.byref(h), B, bad_n, *[ptr(c) for c in cols], None, -1) == capi.E_INVALID
        assert not h.value and lib.ellhip_last_error()
    with pytest.raises(capi.EllHipError):
        gpu.BatchLowpassProblem(129, *cols)   # the LDS engine's constructor keeps its limit
    # the old entry points still refuse a streamed handle, whichever constructor made the oracle
    streamed = gpu.EllBatchStreamed.new_with_scalar(np.full(B, 10.0), x0)
    for entry in ("ellhip_batch_lowpass_optim", "ellhip_batch_lowpass_feas", "ellhip_batch_lowpass_optim_stable",
                  "ellhip_batch_lowpass_feas_stable"):
        refused(streamed, entry)
        refused(streamed, entry, gpu.BatchLowpassProblem(n, *cols))
    assert b"streamed" in lib.ellhip_last_error()
    # and a good pair still runs
    good = new_spaces(gpu, B, n)
    recs = [ref.solve_optim(n, ref.LOOSE, 50, TOL)] * B
    assert_all_equal(prob, good, run_optim(prob, good, [ref.LOOSE] * B, 50), recs, n)


# ---- 10. the C++ mirror -----------------------------------------------------------------------------------------------------------------
def test_cpp_runner_matches_the_cpu_runs(gpu):
    import cpp_build
    exe = cpp_build.build_runner("batch_lowpass_streamed_runner.cpp", "hip")
    got = cpp_build.run_json_lines(exe)
    n, B = 136, 6
    assert len(got) == B
    for b in range(B):
        d, r = got[f"sweep_{b}"], ref.solve_optim(n, ref.family(b))
        assert d["niter"] == r["niter"] and d["status"] == r["status"] and d["has_best"] == 1
        assert d["gamma"] == r["gamma"] and d["x_best"] == r["x_best"].tolist()
        assert (d["idx1"], d["idx2"], d["idx3"], d["kmax"]) == tuple(r["state"][k] for k in ("idx1", "idx2", "idx3", "kmax"))
