"""GPU: the batched device-resident low-pass design loop on a streamed EllStable batch handle
(include/ellhip_batch_lowpass_streamed_stable.h) against the CPU loop (oracle.OracleLowpass over oracle.OracleEllStable,
through tests/batch_stable_loop_reference.py), against the same loop on the LDS engine and against the host-driven form over
ellhip_batch_update.  The kernel follows the reference's statement order, so every comparison is EXACT: float64 bit patterns
(NaN by position) and integers -- niter, status, has_best, gamma, x_best, the oracle state (cursors, kmax, fmax, more_alt,
sp_sq) and the spaces: the packed buffer with its scratch triangle, xc, kappa and tsq.

The pinned counts are those of tests/test_batch_lowpass_streamed_stable_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import batch_lowpass_reference as lp
import batch_stable_loop_reference as ref
from util import random_factor

pytestmark = pytest.mark.gpu

UNCAPPED, TOL = lp.MAX_ITERS, lp.TOL


def same_bits(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind != "f" and b.dtype.kind != "f":
        np.testing.assert_array_equal(a, b, err_msg=what)
        return
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    na = np.isnan(a)
    np.testing.assert_array_equal(na, np.isnan(b), err_msg=what + ": NaN positions")
    np.testing.assert_array_equal(a[~na].view(np.uint64), b[~na].view(np.uint64), err_msg=what + ": bits")


def make_batch(gpu, case, cls=None):
    cls = gpu.EllStableBatchStreamed if cls is None else cls
    if case.mq is None:
        batch = cls.new_with_scalar(case.kappa, case.xc)
    else:
        batch = cls.new_with_matrix(case.kappa, case.mq, case.xc)
    assert batch.variant == gpu.capi.SPACE_ELL_STABLE and (batch.B, batch.n) == (case.B, case.n)
    if not case.use_parallel:
        batch.set_use_parallel_cut(False)
    return batch


def make_gpu(gpu, case, chunk=None):
    prob = gpu.BatchLowpassProblem.streamed(case.n, *lp.columns(case.problems))
    if chunk is not None:
        prob.set_chunk(chunk)
    batch = make_batch(gpu, case)
    assert batch.is_streamed
    return prob, batch


def run_device(prob, batch, case, gamma=None, max_iters=None, tol=None):
    """-> records shaped like the reference's"""
    max_iters = case.max_iters if max_iters is None else max_iters
    tol = case.tol if tol is None else tol
    if case.optim:
        x, has, niter, gamma, status = prob.optim(batch, case.gamma if gamma is None else gamma, max_iters, tol)
    else:
        x, has, niter, status = prob.feas(batch, max_iters, tol)
        gamma = case.gamma
    mq, xc, kappa, tsq = batch.mq, batch.xc(), batch.kappa, batch.tsq()
    st = prob.state()
    states = [{k: st[k][b] for k in lp.STATE_KEYS} for b in range(case.B)]
    for b in range(case.B):  # a row without a result stays as the caller left it
        assert has[b] or np.isnan(x[b]).all()
    return [dict(x_best=x[b] if has[b] else None, niter=int(niter[b]), gamma=gamma[b], status=int(status[b]),
                 state=states[b], mq=mq[b], xc=xc[b], kappa=kappa[b], tsq=tsq[b]) for b in range(case.B)]


def assert_records_equal(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        tag = f"{what} instance {b}"
        assert g["niter"] == w["niter"] and g["status"] == w["status"], (tag, g["niter"], w["niter"], g["status"], w["status"])
        same_bits(g["gamma"], w["gamma"], tag + " gamma")
        assert (g["x_best"] is None) == (w["x_best"] is None), tag + " has_best"
        if w["x_best"] is not None:
            same_bits(g["x_best"], w["x_best"], tag + " x_best")
        assert g["state"].keys() == w["state"].keys()
        for k in w["state"]:
            same_bits(g["state"][k], w["state"][k], f"{tag} {k}")
        for k in ("mq", "xc", "kappa", "tsq"):
            same_bits(g[k], w[k], f"{tag} {k}")


def cpu_records(case):
    """ref.cpu_run, with the CPU loop of equal problems run once when every instance starts as new_with_scalar leaves it"""
    if case.mq is not None or case.xc.any() or (case.kappa != case.kappa[0]).any():
        return ref.cpu_run(case)
    uniq = sorted(set(case.problems))
    gam = {p: case.gamma[case.problems.index(p)] for p in uniq}
    assert all(case.gamma[b] == gam[p] for b, p in enumerate(case.problems))
    one = ref.Case(case.kind, uniq, case.n, case.kappa[0], np.zeros(case.n), max_iters=case.max_iters, tol=case.tol,
                   gamma=[gam[p] for p in uniq], use_parallel=case.use_parallel)
    recs = dict(zip(uniq, ref.cpu_run(one)))
    return [recs[p] for p in case.problems]


def check(gpu, case, chunk=None):
    """the device loop against the CPU loop; -> the CPU records"""
    want = cpu_records(case)
    prob, batch = make_gpu(gpu, case, chunk)
    assert_records_equal(run_device(prob, batch, case), want, f"device loop vs CPU ({case.kind}, n = {case.n})")
    return want


# ---- 1. complete runs against the CPU records ---------------------------------------------------------------------------------
COMPLETE = [
    (lp.EMPTY_TRANSITION, UNCAPPED, (1203, ref.NOSOLN, False), (1203, False)),
    (lp.NO_STOPBAND_B, UNCAPPED, (724, ref.UNKNOWN, False), (724, True)),   # Unknown: niter not advanced by the last round
    (lp.LOOSE, 1500, (1500, ref.SUCCESS, True), (728, True)),               # (optim capped; feas uncapped)
]


@pytest.mark.parametrize("consts,cap,optim,feas", COMPLETE, ids=["empty-transition", "no-stopband", "loose"])
def test_complete_runs(gpu, consts, cap, optim, feas):
    r = check(gpu, ref.lp_case(129, [consts] * 2, max_iters=cap))[0]
    assert (r["niter"], r["status"], r["x_best"] is not None) == optim
    assert r["gamma"] < consts[4] if optim[2] else r["gamma"] == consts[4]
    f = check(gpu, ref.lp_case(129, [consts] * 2, feas=True, max_iters=UNCAPPED))[0]
    assert (f["niter"], f["x_best"] is not None) == feas
    assert f["status"] == (ref.SUCCESS if feas[1] else ref.NOSOLN)


# ---- 2. a mixed batch: stopped instances keep voting while the rest go on -----------------------------------------------------
def test_mixed_batch_stops_at_eight_different_rounds(gpu):
    consts = [lp.family(s) for s in range(6)] + [lp.NO_STOPBAND_B, lp.EMPTY_TRANSITION]
    recs = check(gpu, ref.lp_case(130, consts, max_iters=UNCAPPED))
    assert [r["niter"] for r in recs] == [143, 154, 165, 179, 196, 217, 732, 1220]
    assert [r["status"] for r in recs] == [ref.NOSOLN] * 6 + [ref.UNKNOWN, ref.NOSOLN]
    feas = check(gpu, ref.lp_case(130, consts, feas=True, max_iters=UNCAPPED))
    assert [r["niter"] for r in feas] == [143, 154, 165, 179, 196, 217, 732, 1220]
    assert [r["x_best"] is not None for r in feas] == [False] * 6 + [True, False]


# ---- 3. block shapes, cut off by max_iters ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_iters", [(512, 150), (1023, 40), (193, 300)])
def test_block_shapes(gpu, n, max_iters):
    """8 full waves; a padded last wave; a remainder of both BSS_CHUNK and the back solve's 64-term pieces"""
    r = check(gpu, ref.lp_case(n, [lp.LOOSE] * 2, max_iters=max_iters))[0]
    assert (r["niter"], r["status"], r["x_best"]) == (max_iters, ref.SUCCESS, None)
    # from the identity the factor stays the identity and the scratch triangle holds products with zeros: signed zeros, which
    # the comparison above takes bit by bit
    assert np.signbit(np.tril(r["mq"], -1)).any() and not np.tril(r["mq"], -1).any()
    # so the same shape once more from random factors, where factor and scratch triangle are populated
    want = check(gpu, ref.lp_case(n, [lp.LOOSE, lp.family(2)], max_iters=max_iters).with_random_factors(n))
    assert min(w["niter"] for w in want) >= 18
    assert all(np.count_nonzero(np.tril(w["mq"], -1)) > n * (n - 1) // 2 * 9 // 10 for w in want)


CONSTS_1024 = [lp.LOOSE, lp.LOOSE]


@pytest.fixture(scope="module")
def prob1024(gpu):
    """the n = 1024 table is 240 MiB: one handle for the module"""
    prob = gpu.BatchLowpassProblem.streamed(1024, *lp.columns(CONSTS_1024))
    yield prob
    del prob


def as_new(prob, consts_list):
    """The shared handle as its constructor left it, whatever ran before: assess_optim sets sp_sq to the gamma it is given
    (src/oracles/lowpass_oracle.rs:140), reset() restores the cursors, fmax and kmax."""
    prob.assess_optim(np.zeros((prob.B, prob.n)), np.array([c[4] for c in consts_list]))
    prob.reset()
    prob.set_chunk(256)


@pytest.mark.parametrize("feas", [False, True], ids=["optim", "feas"])
def test_n1024(gpu, prob1024, feas):
    case = ref.lp_case(1024, CONSTS_1024, feas=feas, max_iters=60)
    want = cpu_records(case)
    assert all((w["niter"], w["status"], w["x_best"]) == (60, ref.SUCCESS, None) for w in want)
    as_new(prob1024, CONSTS_1024)
    assert_records_equal(run_device(prob1024, make_batch(gpu, case), case), want, "n = 1024")
    if not feas:  # and from random factors, where factor and scratch triangle are populated
        case = ref.lp_case(1024, CONSTS_1024, max_iters=20).with_random_factors(1024)
        want = ref.cpu_run(case)
        assert all(w["niter"] == 20 for w in want)
        as_new(prob1024, CONSTS_1024)
        assert_records_equal(run_device(prob1024, make_batch(gpu, case), case), want, "n = 1024, random factors")


# ---- 4. against the LDS engine ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feas", [False, True], ids=["optim", "feas"])
@pytest.mark.parametrize("n", [1, 2, 16, 33, 64, 128])
def test_equals_the_lds_engine(gpu, n, feas):
    """ellhip_batch_lowpass_{optim,feas}_stable on an EllStableBatch against the new entry points on an
    EllStableBatchStreamed, from the identity and from random factors with junk in the scratch triangle"""
    consts = [lp.LOOSE, lp.family(0), lp.family(4)]
    cap = 1500 if n <= 33 else 300
    for start in ("identity", "random factors"):
        case = ref.lp_case(n, consts, feas=feas, max_iters=cap)
        if start == "random factors":
            case = case.with_random_factors(700 + n)
        lds = (gpu.BatchLowpassProblem(n, *lp.columns(consts)), make_batch(gpu, case, gpu.EllStableBatch))
        st = make_gpu(gpu, case)
        assert not hasattr(lds[1], "is_streamed") and st[1].is_streamed
        got_l, got_s = run_device(*lds, case), run_device(*st, case)
        assert_records_equal(got_s, got_l, f"streamed vs LDS engine, n = {n}, {start}")
        if n == 1 and start == "identity" and not feas:  # the state turns NaN and the oracle finds nothing to cut with
            assert all(g["status"] == ref.UNKNOWN for g in got_s) and all(np.isnan(g["mq"]).all() for g in got_s)
        if n > 1:  # (n = 2 ends after five rounds, the random-factor starts after nine or more)
            assert max(g["niter"] for g in got_s) >= (5 if n == 2 else 9)


# ---- 5. starts that are not the identity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feas", [False, True], ids=["optim", "feas"])
def test_random_factor_starts(gpu, feas):
    case = ref.lp_case(129, [lp.family(s) for s in range(3)], feas=feas, max_iters=UNCAPPED).with_random_factors(11)
    assert np.count_nonzero(np.tril(case.mq, -1)) == 3 * 129 * 128 // 2   # junk in the scratch triangle
    want = check(gpu, case)
    assert min(w["niter"] for w in want) > 5
    assert all(np.count_nonzero(np.triu(w["mq"], 1)) > 129 * 128 // 2 * 9 // 10 for w in want)   # not a comparison of zeros


def test_from_space_clone(gpu):
    n, B = 129, 3
    rng = np.random.default_rng(66)
    base = gpu.EllStable.new_with_matrix(lp.KAPPA, random_factor(n, 67), np.zeros(n))
    for _ in range(5):
        assert int(base._update(0, (rng.standard_normal(n), 0.01))) == 0
    batch = gpu.EllStableBatchStreamed.from_space(base, B)
    assert batch.is_streamed and batch.variant == gpu.capi.SPACE_ELL_STABLE
    consts = [lp.family(s) for s in range(B)]
    case = ref.Case("lp_optim", consts, n, base.kappa, base.xc(), np.broadcast_to(base.mq, (B, n, n)), max_iters=UNCAPPED,
                    tol=TOL)
    want = ref.cpu_run(case)
    assert min(w["niter"] for w in want) > 5
    prob = gpu.BatchLowpassProblem.streamed(n, *lp.columns(consts))
    assert_records_equal(run_device(prob, batch, case), want, "from_space")


# ---- 6. launch structure ----------------------------------------------------------------------------------------------------------
SHAPE_N, SHAPE_CONSTS = 129, [lp.family(1), lp.NO_STOPBAND_B]


def shape_case(**kw):
    return ref.lp_case(SHAPE_N, SHAPE_CONSTS, **{"max_iters": UNCAPPED, **kw})


@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunking_changes_nothing(gpu, chunk):
    want = check(gpu, shape_case(), chunk=chunk)
    assert [w["niter"] for w in want] == [153, 724]


def test_max_iters_zero_moves_nothing(gpu):
    case = shape_case().with_random_factors(5)
    prob, batch = make_gpu(gpu, case)
    before = (batch.mq, batch.xc(), batch.kappa, batch.tsq(), prob.state())
    x_best, has, niter, gamma, status = prob.optim(batch, 0.05, 0, TOL)
    assert (niter == 0).all() and (has == 0).all() and (status == ref.SUCCESS).all() and np.isnan(x_best).all()
    assert (gamma == 0.05).all()
    after = (batch.mq, batch.xc(), batch.kappa, batch.tsq(), prob.state())
    for a, b in zip(before[:4], after[:4]):
        same_bits(a, b, "max_iters = 0")
    for k in lp.STATE_KEYS:
        same_bits(before[4][k], after[4][k], k)


def live_pairs(case):
    return [(ref._oracle(case, b), ref.cpu_space(case, b)) for b in range(case.B)]


def cpu_record(omega, space, out):
    x, niter, gamma, status = out
    return dict(x_best=None if x is None else np.array(x), niter=niter, gamma=gamma, status=status, state=omega.state(),
                **ref.space_record(space))


def test_cut_off_continue_and_reset(gpu):
    case = shape_case()
    full = cpu_records(case)
    pairs = live_pairs(case)
    first = [cpu_record(o, s, o.cutting_plane_optim(s, g, 100, TOL)) for (o, s), g in zip(pairs, case.gamma)]
    assert all(r["niter"] == 100 and r["status"] == ref.SUCCESS for r in first)
    prob, batch = make_gpu(gpu, case)
    got = run_device(prob, batch, case, max_iters=100)
    assert_records_equal(got, first, "cut off at 100")
    second = [cpu_record(o, s, o.cutting_plane_optim(s, r["gamma"], UNCAPPED, TOL)) for (o, s), r in zip(pairs, first)]
    for r, f in zip(second, full):  # the CPU run driven this way is the uninterrupted run
        assert r["niter"] + 100 == f["niter"] and r["status"] == f["status"] and r["state"] == f["state"]
        assert np.array_equal(r["mq"], f["mq"]) and np.array_equal(r["xc"], f["xc"])
    got2 = run_device(prob, batch, case, gamma=np.array([g["gamma"] for g in got]))
    assert_records_equal(got2, second, "continued")
    # reset: cursors, fmax and kmax as after new(); a rerun from fresh spaces reproduces the whole run
    prob.reset()
    s = prob.state()
    np.testing.assert_array_equal(s["idx1"], np.full(case.B, -1))
    np.testing.assert_array_equal(s["idx2"], s["nwpass"] - 1)
    np.testing.assert_array_equal(s["idx3"], s["nwstop"] - 1)
    assert (s["fmax"] == -np.inf).all() and (s["kmax"] == -1).all() and (s["more_alt"] == 1).all()
    assert_records_equal(run_device(prob, make_batch(gpu, case), case), full, "after reset")


def test_batch_update_between_two_loops(gpu):
    case = shape_case()
    B, n = case.B, case.n
    prob, batch = make_gpu(gpu, case)
    pairs = live_pairs(case)
    first = [cpu_record(o, s, o.cutting_plane_optim(s, g, 60, TOL)) for (o, s), g in zip(pairs, case.gamma)]
    got = run_device(prob, batch, case, max_iters=60)
    assert_records_equal(got, first, "first loop")
    rng = np.random.default_rng(3)
    grads = rng.standard_normal((1, B, n))
    kinds = np.array([[0, 1]], dtype=np.int32)
    beta = np.zeros((1, B))
    want = np.zeros((1, B), dtype=np.int32)
    for b, (_, space) in enumerate(pairs):
        beta[0, b] = 0.1 * np.sqrt(space.tsq) if kinds[0, b] == 0 else 0.0
        want[0, b] = space.update(int(kinds[0, b]), grads[0, b], beta[0, b])
    status, _ = batch.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    assert (want == 0).all()
    for b, (_, space) in enumerate(pairs):
        same_bits(batch.mq[b], space.mq, "mq after the update between the loops")
    second = [cpu_record(o, s, o.cutting_plane_optim(s, r["gamma"], 400, TOL)) for (o, s), r in zip(pairs, first)]
    got2 = run_device(prob, batch, case, gamma=np.array([g["gamma"] for g in got]), max_iters=400)
    assert_records_equal(got2, second, "second loop")


def test_tolerance_stop(gpu):
    """a tolerance taken from the CPU run's own tsq sequence: the first round from 20 on whose tsq is a new minimum.  The
    round that meets it completes its update and is not counted."""
    case = shape_case()
    omega, space = live_pairs(case)[0]
    gamma, tsq = case.gamma[0], []
    for _ in range(150):
        _, niter, gamma, status = omega.cutting_plane_optim(space, gamma, 1, 0.0)
        assert niter == 1 and status == ref.SUCCESS
        tsq.append(space.tsq)
    k = next(k for k in range(20, 150) if tsq[k] < min(tsq[:k]))
    tol = 0.5 * (tsq[k] + min(tsq[:k]))
    rec = check(gpu, shape_case(tol=tol))[0]
    assert rec["niter"] == k and rec["status"] == ref.SUCCESS and rec["tsq"] == tsq[k] < tol


# ---- 7. options -------------------------------------------------------------------------------------------------------------------
def test_without_parallel_cuts(gpu):
    consts = [lp.LOOSE, lp.family(1)]
    plain = cpu_records(ref.lp_case(129, consts, max_iters=300))
    want = check(gpu, ref.lp_case(129, consts, max_iters=300, use_parallel=False))
    assert any(a["niter"] != b["niter"] or not np.array_equal(a["xc"], b["xc"]) for a, b in zip(plain, want))
    batch = make_batch(gpu, ref.lp_case(129, consts))
    assert not hasattr(batch, "set_no_defer_trick")
    assert gpu.capi.load().ellhip_batch_set_no_defer_trick(batch._h, 1) == gpu.capi.E_INVALID


# ---- 8. the host-driven form as the independent second check ----------------------------------------------------------------------
@pytest.mark.parametrize("feas", [False, True], ids=["optim", "feas"])
def test_equals_the_host_driven_form(gpu, feas):
    case = ref.lp_case(129, [lp.family(s) for s in range(3)], feas=feas, max_iters=UNCAPPED).with_random_factors(23)
    prob, batch = make_gpu(gpu, case)
    got = run_device(prob, batch, case)
    hosted = ref.host_driven(make_batch(gpu, case), case)
    assert min(h["niter"] for h in hosted) > 5
    assert_records_equal(got, hosted, "device loop vs host-driven")


# ---- 9. more workgroups than CUs --------------------------------------------------------------------------------------------------
def test_six_hundred_workgroups(gpu):
    want = check(gpu, ref.lp_case(129, [lp.family(b % 6) for b in range(600)], max_iters=40))
    assert all(w["niter"] == 40 and w["status"] == ref.SUCCESS for w in want)


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_spaces_untouched(gpu):
    capi = gpu.capi
    lib = capi.load()
    n, B = 16, 3
    cols = lp.columns([lp.LOOSE] * B)
    prob = gpu.BatchLowpassProblem.streamed(n, *cols)
    rng = np.random.default_rng(2)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def stable_args(BB, nn):
        return (np.full(BB, 10.0), np.stack([random_factor(nn, 7 + b) for b in range(BB)]), rng.standard_normal((BB, nn)))

    def refused(batch, entry, problem=prob, null=None):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        state = problem.state()
        gamma = np.full(batch.B, 0.3)
        xb = np.full((batch.B, batch.n), np.nan)
        has = np.full(batch.B, -5, dtype=np.int32)
        niter = np.full(batch.B, -5, dtype=np.int64)
        status = np.full(batch.B, -5, dtype=np.int32)
        args = dict(spaces=batch._h, o=problem._h, gamma=ptr(gamma), max_iters=100, tol=1e-10, x=ptr(xb), has=ptr(has),
                    niter=ptr(niter), status=ptr(status))
        if "optim" not in entry:
            del args["gamma"]
        if null is not None:
            args[null] = None
        assert getattr(lib, entry)(*args.values()) == capi.E_INVALID and lib.ellhip_last_error(), (entry, null)
        for a, b, what in zip(before, (batch.mq, batch.xc(), batch.kappa, batch.tsq()), ("mq", "xc", "kappa", "tsq")):
            same_bits(a, b, f"{entry}: {what} untouched")
        after = problem.state()
        for k in lp.STATE_KEYS:
            same_bits(state[k], after[k], f"{entry}: oracle {k} untouched")
        assert np.isnan(xb).all() and (gamma == 0.3).all()
        assert (has == -5).all() and (niter == -5).all() and (status == -5).all()

    for entry in capi.BATCH_LOWPASS_STREAMED_STABLE_EXPORTS:
        refused(gpu.EllBatchStreamed.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n))), entry)   # streamed Ell
        refused(gpu.EllStableBatch.new_with_matrix(*stable_args(B, n)), entry)                                # LDS EllStable
        refused(gpu.EllBatch.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n))), entry)           # LDS Ell
        refused(gpu.EllStableBatchStreamed.new_with_matrix(*stable_args(B + 1, n)), entry)                    # wrong B
        refused(gpu.EllStableBatchStreamed.new_with_matrix(*stable_args(B, n + 1)), entry)                    # wrong n
        refused(gpu.EllStableBatchStreamed.new_with_matrix(*stable_args(B, n)), entry, gpu.BatchLowpassProblem(n + 1, *cols))
        good = gpu.EllStableBatchStreamed.new_with_matrix(*stable_args(B, n))
        for null in ("spaces", "o", "has", "niter", "status") + (("gamma",) if "optim" in entry else ()):
            refused(good, entry, null=null)
        if lib.ellhip_device_count() > 1:   # the oracle on another device
            refused(good, entry, gpu.BatchLowpassProblem.streamed(n, *cols, device=1))
    # the Python mirror reaches the new entry points by the handle's kind, and says which one refused
    with pytest.raises(capi.EllHipError, match="ellhip_batch_lowpass_optim_streamed_stable.*differ in B or n"):
        prob.optim(gpu.EllStableBatchStreamed.new_with_scalar(np.full(B + 1, 10.0), np.zeros((B + 1, n))), 0.3, 10, TOL)
    # and a good pair still runs, with an oracle handle of either constructor
    case = ref.lp_case(n, [lp.LOOSE] * B, max_iters=50).with_random_factors(9)
    want = ref.cpu_run(case)
    assert_records_equal(run_device(prob, make_batch(gpu, case), case), want, "a good pair")
    small = gpu.BatchLowpassProblem(n, *cols)
    assert_records_equal(run_device(small, make_batch(gpu, case), case), want, "an oracle handle of the LDS constructor")


# ---- 11. the C++ mirror -----------------------------------------------------------------------------------------------------------
def test_cpp_runner_matches_the_cpu_runs(gpu):
    import cpp_build
    exe = cpp_build.build_runner("batch_lowpass_streamed_stable_runner.cpp", "hip")
    got = cpp_build.run_json_lines(exe)
    n = 130
    consts = [lp.family(s) for s in range(6)] + [lp.LOOSE]
    B = len(consts)
    assert len(got) == 2 * B
    want = ref.cpu_run(ref.lp_case(n, consts, max_iters=1500))
    assert want[6]["niter"] == 1500 and want[6]["x_best"] is not None
    for b, r in enumerate(want):
        d = got[f"sweep_{b}"]
        assert d["niter"] == r["niter"] and d["status"] == r["status"] and d["has_best"] == (r["x_best"] is not None)
        assert d["gamma"] == r["gamma"]
        if r["x_best"] is not None:
            assert d["x_best"] == r["x_best"].tolist()
        assert (d["idx1"], d["idx2"], d["idx3"], d["kmax"]) == tuple(r["state"][k] for k in ("idx1", "idx2", "idx3", "kmax"))
    # the feas run follows a reset: sp_sq is what the optim run left, the last gamma it was handed
    again = [c[:4] + (w["gamma"],) for c, w in zip(consts, want)]
    for b, r in enumerate(ref.cpu_run(ref.lp_case(n, again, feas=True, max_iters=1500))):
        d = got[f"feas_{b}"]
        assert (d["niter"], d["status"], d["has_best"]) == (r["niter"], r["status"], int(r["x_best"] is not None)), b
