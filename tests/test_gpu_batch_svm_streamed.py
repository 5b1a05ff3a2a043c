"""GPU: the batched device-resident SVM loop on streamed batch handles (include/ellhip_batch_svm_streamed.h), Ell and
EllStable, against the reference's SvmOracle restated in tests/svm_reference.py, its cutting_plane_optim over the CPU oracle's
spaces (tests/batch_svm_reference.py, tests/batch_stable_loop_reference.py) and the same loop on the LDS engine.  The device
folds every margin like the CPU and picks the sample by the reference's scan rule, so every comparison is EXACT: float64 bit
patterns (the sign of a zero counts; NaN is compared by position) and integers -- margins, gradient, beta, gamma, min_idx /
min_val, x_best, has_best, niter, status and the spaces' matrix (EllStable: the packed buffer, scratch triangle included),
xc, kappa and tsq afterwards.

The pinned counts are those of tests/test_batch_svm_streamed_cpu.py, whose cached records are used here."""
import ctypes as C
import struct

import numpy as np
import pytest

import batch_svm_reference as ref
import svm_reference as svm
import test_batch_svm_streamed_cpu as pins
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INF = np.inf
TOL = pins.TOL
LABELS = np.array([-7, -1, 0, 1, 7], dtype=np.int32)
SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]


def same_bits(a, b):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def assert_bits(got, want, what):
    assert same_bits(got, want), (what, got, want)


def new_spaces(gpu, stable, B, n, streamed=True):
    cls = {(False, True): gpu.EllBatchStreamed, (True, True): gpu.EllStableBatchStreamed,
           (False, False): gpu.EllBatch, (True, False): gpu.EllStableBatch}[(stable, streamed)]
    batch = cls.new_with_scalar(np.full(B, ref.KAPPA), np.zeros((B, n)))
    assert bool(getattr(batch, "is_streamed", False)) == streamed
    assert batch.variant == (gpu.capi.SPACE_ELL_STABLE if stable else gpu.capi.SPACE_ELL)
    return batch


def cpu_space(stable, n):
    return (O.OracleEllStable if stable else O.OracleEll).new_with_scalar(ref.KAPPA, np.zeros(n))


def table(data, b):
    return data if data.ndim == 2 else data[b]


def family_arrays(members, m, nfeat):
    sets = [ref.family(s, m, nfeat) for s in members]
    return np.stack([X for X, _ in sets]), np.stack([l for _, l in sets])


def assert_runs_equal(got, recs, n):
    x_best, has, niter, gamma, status = got
    np.testing.assert_array_equal(niter, np.array([r["niter"] for r in recs], dtype=np.int64))
    np.testing.assert_array_equal(status, np.array([r["status"] for r in recs], dtype=np.int32))
    np.testing.assert_array_equal(has, np.array([r["x_best"] is not None for r in recs], dtype=np.int32))
    assert_bits(gamma, np.array([r["gamma"] for r in recs]), "gamma")
    want = np.stack([np.full(n, np.nan) if r["x_best"] is None else r["x_best"] for r in recs])
    assert_bits(x_best, want, "x_best")   # rows without a result stay as the caller left them (NaN)


def assert_state_equal(prob, batch, recs):
    idx, val = prob.last()
    np.testing.assert_array_equal(idx, np.array([r["min_idx"] for r in recs], dtype=np.int64))
    assert_bits(val, np.array([r["min_val"] for r in recs]), "min_val")
    assert_bits(batch.mq, np.stack([r["mq"] for r in recs]), "mq")
    assert_bits(batch.xc(), np.stack([r["xc"] for r in recs]), "xc")
    assert_bits(batch.kappa, np.array([r["kappa"] for r in recs]), "kappa")
    assert_bits(batch.tsq(), np.array([r["tsq"] for r in recs]), "tsq")


def check_loop(gpu, stable, data, lab, recs, max_iters, tol, chunk=None, batch=None, prob=None):
    B, n = lab.shape[0], data.shape[-1] + 1
    prob = gpu.BatchSvmProblem.streamed(data, lab) if prob is None else prob
    if chunk is not None:
        prob.set_chunk(chunk)
    batch = new_spaces(gpu, stable, B, n) if batch is None else batch
    got = prob.optim(batch, INF, max_iters, tol)
    assert_runs_equal(got, recs, n)
    assert_state_equal(prob, batch, recs)
    return prob, batch, got


def check_family(gpu, stable, m, nfeat, members, max_iters, tol=TOL, chunk=None):
    data, lab = family_arrays(members, m, nfeat)
    recs = [pins.record(stable, s, m, nfeat, max_iters, tol) for s in members]
    return recs, check_loop(gpu, stable, data, lab, recs, max_iters, tol, chunk)


# ---- 1. the oracle call by call ---------------------------------------------------------------------------------------------
def check_calls(prob, data, lab, x):
    """margins, assess_optim and last of every problem at x [B][n] against svm_reference"""
    B = lab.shape[0]
    mg = prob.margins(x)
    grad, beta, gamma = prob.assess_optim(x)
    idx, val = prob.last()
    for b in range(B):
        X = table(data, b)
        assert_bits(mg[b], svm.margins(X, lab[b], x[b]), f"margins {b}")
        (rg, rb), _, rgamma, ridx, rval = svm.assess_optim(X, lab[b], x[b])
        assert idx[b] == ridx and same_bits(val[b], rval), (b, idx[b], val[b], ridx, rval)
        assert_bits(grad[b], rg, f"grad {b}")
        assert same_bits(beta[b], rb) and same_bits(gamma[b], rgamma), (b, beta[b], gamma[b], rb, rgamma)
    return idx, val


# m < n (most threads hold no sample, ld padding); m = n; m = n + 1; T = 192 exactly, with stride; n = 193 in T = 256 with
# inactive threads; the largest blocks
CALL_SHAPES = [(5, 128, 3), (129, 128, 2), (130, 128, 2), (400, 191, 2), (70, 192, 2), (33, 1022, 2), (1100, 1023, 2)]


@pytest.mark.parametrize("m,nfeat,B", CALL_SHAPES)
def test_oracle_call_by_call(gpu, m, nfeat, B):
    rng = np.random.default_rng(1000 * m + nfeat)
    data = rng.standard_normal((B, m, nfeat))
    lab = rng.choice(LABELS, size=(B, m))
    per = gpu.BatchSvmProblem.streamed(data, lab)
    shared = gpu.BatchSvmProblem.streamed(data[B - 1], lab)
    assert per.n == nfeat + 1 and not per.shared and shared.shared
    idx, val = per.last()   # as after new(): nothing scanned yet
    assert not idx.any() and (val == INF).all()
    for _ in range(2):
        x = rng.standard_normal((B, nfeat + 1))
        check_calls(per, data, lab, x)
        check_calls(shared, data[B - 1], lab, x)
    # margins() looks without touching what last() reports
    kept = per.last()
    per.margins(rng.standard_normal((B, nfeat + 1)))
    assert np.array_equal(per.last()[0], kept[0]) and same_bits(per.last()[1], kept[1])
    # an all-NaN x: nothing is below +inf -> (0, +inf), the zero cut, gamma = +0.0
    grad, beta, gamma = per.assess_optim(np.full((B, nfeat + 1), np.nan))
    assert_bits(grad, np.zeros((B, nfeat + 1)), "grad")
    assert same_bits(beta, np.zeros(B)) and same_bits(gamma, np.zeros(B))
    idx, val = per.last()
    assert not idx.any() and (val == INF).all()


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------
def test_duplicate_rows_first_index_wins_wide(gpu):
    """n = 129 in a block of 192: later copies of the winning row in another wave, in the winner's own stride and both"""
    m, nfeat, B = 300, 128, 3
    rng = np.random.default_rng(3)
    data = rng.standard_normal((B, m, nfeat))
    lab = np.ones((B, m), dtype=np.int32)
    x = rng.standard_normal((B, nfeat + 1))
    want = []
    for b in range(B):
        r = svm.argmin(svm.margins(data[b], lab[b], x[b]))[0]
        dup = [(r + 70) % m, (r + 129) % m, (r + 199) % m]
        data[b, dup] = data[b, r]
        want.append(min([r] + dup))
    prob = gpu.BatchSvmProblem.streamed(data, lab)
    check_calls(prob, data, lab, x)
    assert prob.last()[0].tolist() == want


# (first, second): the second zero in the first one's own stride (thread 4); in another wave (thread 100); the earlier index
# in the higher-numbered thread and the later wave (thread 70 against thread 1's second sample)
@pytest.mark.parametrize("first,second", [(4, 133), (4, 100), (70, 130)])
def test_signed_zero_and_duplicate_ties_wide(gpu, first, second):
    """n = 129: every margin is 5 except indices `first` and `second`, zeros of opposite sign, in both orders (problems 0 and
    1).  The first index wins with its own bits."""
    m, nfeat = 140, 128
    data = np.zeros((m, nfeat))
    data[:, 0] = 5.0
    data[first, 0] = data[second, 0] = 0.0
    lab = np.ones((2, m), dtype=np.int32)
    lab[0, first], lab[0, second] = -1, 1
    lab[1, first], lab[1, second] = 1, -1
    prob = gpu.BatchSvmProblem.streamed(data, lab)     # one shared table, the labels differ
    x = np.zeros((2, nfeat + 1))
    x[:, 0] = 1.0
    check_calls(prob, data, lab, x)
    idx, val = prob.last()
    assert idx.tolist() == [first, first] and (val == 0.0).all()
    assert np.signbit(val).tolist() == [True, False]
    grad, beta, gamma = prob.assess_optim(x)
    assert np.signbit(beta).tolist() == [True, False] and np.signbit(gamma).tolist() == [True, False]


# ---- 3. the pinned runs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("shape,max_iters,ell,stb", pins.PINS, ids=pins.PIN_IDS)
def test_pinned_runs(gpu, stable, shape, max_iters, ell, stb):
    """every pinned row as the middle problem of a batch of three, beside the family members s + 3 and s + 6 (the same kind:
    separable or not)"""
    m, nfeat, s = shape
    recs, _ = check_family(gpu, stable, m, nfeat, (s + 3, s, s + 6), max_iters)
    niter, zero, gamma, min_idx = stb if stable else ell
    r = recs[1]
    assert r["niter"] == niter and (min_idx is None or r["min_idx"] == min_idx)
    if zero:
        assert np.isnan(r["xc"]).all() and r["tsq"] == 0.0 and same_bits(r["gamma"], 0.0)
    else:
        assert r["gamma"] == gamma


# ---- 4. the LDS engine ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("n", [2, 3, 64, 65, 128])
def test_equals_the_lds_engine(gpu, stable, n):
    """the same oracle data and the same start on both engines; an oracle handle of either constructor serves both"""
    m, nfeat, B, max_iters, tol = 50, n - 1, 4, 60, 1e-10
    data, lab = family_arrays(range(B), m, nfeat)
    recs = [ref.run(data[b], lab[b], max_iters, tol, space=cpu_space(stable, n)) for b in range(B)]
    assert n == 128 or len({r["niter"] for r in recs}) > 1   # (at n = 128 all four are cut off)
    lds_prob = gpu.BatchSvmProblem(data, lab)
    lds = new_spaces(gpu, stable, B, n, streamed=False)
    want = lds_prob.optim(lds, INF, max_iters, tol)
    assert_runs_equal(want, recs, n)
    assert_state_equal(lds_prob, lds, recs)
    for prob in (gpu.BatchSvmProblem.streamed(data, lab), gpu.BatchSvmProblem(data, lab)):
        batch = new_spaces(gpu, stable, B, n)
        got = prob.optim(batch, INF, max_iters, tol)
        for g, w, what in zip(got, want, ("x_best", "has_best", "niter", "gamma", "status")):
            assert_bits(g, w, what) if g.dtype == np.float64 else np.testing.assert_array_equal(g, w, err_msg=what)
        for g, w in zip(prob.last(), lds_prob.last()):
            assert_bits(g.astype(np.float64), w.astype(np.float64), "last")
        for g, w, what in ((batch.mq, lds.mq, "mq"), (batch.xc(), lds.xc(), "xc"), (batch.kappa, lds.kappa, "kappa"),
                           (batch.tsq(), lds.tsq(), "tsq")):
            assert_bits(g, w, what)
    # a streamed-constructor handle of n <= 128 on the LDS engine
    again = new_spaces(gpu, stable, B, n, streamed=False)
    prob = gpu.BatchSvmProblem.streamed(data, lab)
    assert_runs_equal(prob.optim(again, INF, max_iters, tol), recs, n)
    assert_state_equal(prob, again, recs)


# ---- 5. stops ---------------------------------------------------------------------------------------------------------------
def test_mixed_batch_stops_at_different_iterations(gpu):
    m, nfeat, members, max_iters = pins.MIXED
    recs, _ = check_family(gpu, False, m, nfeat, members, max_iters)
    assert tuple(r["niter"] for r in recs) == pins.MIXED_NITER
    check_family(gpu, True, m, nfeat, members, max_iters)


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunking_changes_nothing(gpu, stable, chunk):
    """chunk 1: the early oracle call is never made and no sweep is fused; 7: six fused rounds, then a plain one; 256: one
    launch.  s = 0 ends on its zero cut inside the run, the others are cut off."""
    recs, _ = check_family(gpu, stable, 200, 129, (0, 1, 2), 120, chunk=chunk)
    assert recs[0]["niter"] == (98 if stable else 100) and recs[1]["niter"] == 120


@pytest.mark.parametrize("stable", SPACES)
def test_cut_off_and_resume(gpu, stable):
    m, nfeat, B, more = 200, 129, 3, 150
    n = nfeat + 1
    data, lab = family_arrays(range(B), m, nfeat)
    spaces = [cpu_space(stable, n) for _ in range(B)]
    first = [ref.run(data[b], lab[b], 17, TOL, space=spaces[b]) for b in range(B)]
    assert [r["niter"] for r in first] == [17] * B
    prob, batch, got = check_loop(gpu, stable, data, lab, first, 17, TOL)
    # the second call carries on: gamma and last() carry over, x_best starts empty
    second = [ref.run(data[b], lab[b], more, TOL, space=spaces[b], gamma=first[b]["gamma"],
                      last=(first[b]["min_idx"], first[b]["min_val"])) for b in range(B)]
    full = pins.record(stable, 0, m, nfeat, 400)
    assert second[0]["niter"] + 17 == full["niter"] and same_bits(second[0]["mq"], full["mq"])   # the uninterrupted run
    got2 = prob.optim(batch, got[3], more, TOL)
    assert_runs_equal(got2, second, n)
    assert_state_equal(prob, batch, second)


@pytest.mark.parametrize("stable", SPACES)
def test_max_iters_zero_moves_nothing(gpu, stable):
    m, nfeat, B = 200, 129, 3
    n = nfeat + 1
    data, lab = family_arrays(range(B), m, nfeat)
    first = [pins.record(stable, s, m, nfeat, 9) for s in range(B)]
    prob, batch, got = check_loop(gpu, stable, data, lab, first, 9, TOL)
    x_best, has, niter, gamma, status = prob.optim(batch, got[3], 0, TOL)
    assert not has.any() and not niter.any() and not status.any() and np.isnan(x_best).all()
    assert_bits(gamma, got[3], "gamma")
    assert_state_equal(prob, batch, first)


@pytest.mark.parametrize("stable", SPACES)
def test_tol_zero_runs_past_the_zero_cut(gpu, stable):
    """(40, 128), s = 0: 53 rounds, the zero cut, then 5 rounds more with a NaN space (on Ell through the fused sweep)"""
    m, nfeat, max_iters = 40, 128, 59
    recs, _ = check_family(gpu, stable, m, nfeat, (0, 3, 6), max_iters, tol=0.0)
    r = recs[0]
    assert pins.record(stable, 0, m, nfeat, 400)["niter"] == 53
    assert r["niter"] == max_iters and (r["min_idx"], r["min_val"]) == (0, INF)
    assert np.isnan(r["xc"]).all() and np.isnan(r["tsq"]) and same_bits(r["gamma"], 0.0)


# ---- 6. starts, flags and interoperation ------------------------------------------------------------------------------------
def test_non_symmetric_start(gpu):
    """Ell, n = 129: the first round takes the mirror sweep (the product by rows), later ones the fused sweep"""
    m, nfeat, B, max_iters = 200, 128, 3, 30
    n = nfeat + 1
    rng = np.random.default_rng(219)
    data, lab = family_arrays(range(B), m, nfeat)
    kappa = np.full(B, ref.KAPPA)
    mq = np.stack([np.eye(n) * (1.0 + rng.random()) + (0.1 / n) * rng.standard_normal((n, n)) for _ in range(B)])
    assert not np.array_equal(mq, np.swapaxes(mq, 1, 2))
    batch = gpu.EllBatchStreamed.new_with_matrix(kappa, mq, np.zeros((B, n)))
    recs = [ref.run(data[b], lab[b], max_iters, TOL, space=O.OracleEll.new_with_matrix(kappa[b], mq[b], np.zeros(n)))
            for b in range(B)]
    assert [r["niter"] for r in recs] == [max_iters] * B
    check_loop(gpu, False, data, lab, recs, max_iters, TOL, batch=batch)
    q = batch.mq
    assert_bits(q, np.swapaxes(q, 1, 2), "mirrored")
    # one round only: the mirror sweep alone
    batch = gpu.EllBatchStreamed.new_with_matrix(kappa, mq, np.zeros((B, n)))
    one = [ref.run(data[b], lab[b], 1, TOL, space=O.OracleEll.new_with_matrix(kappa[b], mq[b], np.zeros(n))) for b in range(B)]
    check_loop(gpu, False, data, lab, one, 1, TOL, batch=batch)


@pytest.mark.parametrize("stable", SPACES)
def test_batch_update_between_two_loops(gpu, stable):
    m, nfeat, B = 200, 129, 4
    n = nfeat + 1
    data, lab = family_arrays([1, 2, 4, 5], m, nfeat)
    spaces = [cpu_space(stable, n) for _ in range(B)]
    first = [ref.run(data[b], lab[b], 30, TOL, space=spaces[b]) for b in range(B)]
    prob, batch, got = check_loop(gpu, stable, data, lab, first, 30, TOL)
    rng = np.random.default_rng(3)
    grads = rng.standard_normal((1, B, n))
    kinds = rng.integers(0, 2, size=(1, B)).astype(np.int32)
    beta = np.zeros((1, B))
    want = np.zeros((1, B), dtype=np.int32)
    for b, space in enumerate(spaces):
        beta[0, b] = 0.1 * np.sqrt(space.tsq) if kinds[0, b] == 0 else 0.0
        want[0, b] = space.update(int(kinds[0, b]), grads[0, b], beta[0, b])
    status, _ = batch.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    after = [dict(first[b], **ref.space_record(spaces[b])) for b in range(B)]
    assert_state_equal(prob, batch, after)
    second = [ref.run(data[b], lab[b], 60, TOL, space=spaces[b], gamma=first[b]["gamma"]) for b in range(B)]
    assert_runs_equal(prob.optim(batch, got[3], 60, TOL), second, n)
    assert_state_equal(prob, batch, second)


@pytest.mark.parametrize("stable", SPACES)
def test_from_space_clone(gpu, stable):
    m, nfeat, B, max_iters = 200, 129, 3, 50
    n = nfeat + 1
    data, lab = family_arrays(range(B), m, nfeat)
    recs = [pins.record(stable, s, m, nfeat, max_iters) for s in range(B)]
    if stable:
        batch = gpu.EllStableBatchStreamed.from_space(gpu.EllStable.new_with_scalar(ref.KAPPA, np.zeros(n)), B)
    else:
        batch = gpu.EllBatchStreamed.from_space(gpu.Ell.new_with_scalar(ref.KAPPA, np.zeros(n)), B)
    assert batch.is_streamed
    check_loop(gpu, stable, data, lab, recs, max_iters, TOL, batch=batch)


@pytest.mark.parametrize("flag", ["no_defer_trick"])
def test_flags(gpu, flag):
    m, nfeat, B, max_iters = 200, 129, 3, 60
    n = nfeat + 1
    data, lab = family_arrays(range(B), m, nfeat)
    batch = new_spaces(gpu, False, B, n)
    batch.set_no_defer_trick(True)
    spaces = [cpu_space(False, n) for _ in range(B)]
    for space in spaces:
        space.set_no_defer_trick(True)
    recs = [ref.run(data[b], lab[b], max_iters, TOL, space=spaces[b]) for b in range(B)]
    plain = pins.record(False, 1, m, nfeat, max_iters)
    assert not np.array_equal(recs[1]["mq"], plain["mq"])   # the flag does something
    check_loop(gpu, False, data, lab, recs, max_iters, TOL, batch=batch)


# ---- 7. more workgroups than the card holds at once -------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-problem"])
def test_large_population(gpu, shared):
    """B = 600 at (64, 128), 5 iterations: twelve different problems, each fifty times"""
    m, nfeat, B, distinct, max_iters = 64, 128, 600, 12, 5
    data, lab = family_arrays(range(distinct), m, nfeat)
    if shared:   # one table, the labels of member b with a few of them flipped
        data = data[0]
        flip = np.random.default_rng(77).random((distinct, m)) < 0.05
        lab = np.where(flip, -lab, lab).astype(np.int32)
    recs = [ref.run(table(data, b), lab[b], max_iters, TOL) for b in range(distinct)]
    reps = B // distinct
    data_all = data if shared else np.tile(data, (reps, 1, 1))
    check_loop(gpu, False, data_all, np.tile(lab, (reps, 1)), recs * reps, max_iters, TOL)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_spaces_untouched(gpu):
    lib = gpu.capi.load()
    m, nfeat, B = 50, 63, 3
    n = nfeat + 1
    data, lab = family_arrays(range(B), m, nfeat)
    prob = gpu.BatchSvmProblem.streamed(data, lab)
    rng = np.random.default_rng(2)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def refused(entry, batch, oracle=prob, null=None):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        gamma = np.full(batch.B, 0.3)
        xb = np.full((batch.B, batch.n), np.nan)
        has = np.full(batch.B, -5, dtype=np.int32)
        niter = np.full(batch.B, -5, dtype=np.int64)
        status = np.full(batch.B, -5, dtype=np.int32)
        args = dict(gamma=gamma, has=has, niter=niter, status=status)
        if null is not None:
            args[null] = None
        rc = getattr(lib, entry)(batch._h if null != "spaces" else None, oracle._h if null != "oracle" else None,
                                 ptr(args["gamma"]), 100, 1e-10, ptr(xb), ptr(args["has"]), ptr(args["niter"]), ptr(args["status"]))
        assert rc == gpu.capi.E_INVALID and lib.ellhip_last_error(), (entry, null)
        for a, b in zip(before, (batch.mq, batch.xc(), batch.kappa, batch.tsq())):
            assert same_bits(a, b)
        assert np.isnan(xb).all() and (gamma == 0.3).all()
        assert (has == -5).all() and (niter == -5).all() and (status == -5).all()

    def spaces(stable, streamed, B=B, n=n):
        cls = {(False, True): gpu.EllBatchStreamed, (True, True): gpu.EllStableBatchStreamed,
               (False, False): gpu.EllBatch, (True, False): gpu.EllStableBatch}[(stable, streamed)]
        return cls.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n)))

    ell, stable = "ellhip_batch_svm_optim_streamed", "ellhip_batch_svm_optim_streamed_stable"
    refused(ell, spaces(False, False))            # LDS handles
    refused(ell, spaces(True, False))
    refused(stable, spaces(True, False))
    refused(stable, spaces(False, False))
    refused(ell, spaces(True, True))              # the wrong variant
    refused(stable, spaces(False, True))
    for entry, st in ((ell, False), (stable, True)):
        refused(entry, spaces(st, True, B=B + 1))     # wrong B
        refused(entry, spaces(st, True, n=n + 1))     # wrong n
        refused(entry, spaces(st, True, n=nfeat))     # n = nfeat
        for null in ("spaces", "oracle", "gamma", "has", "niter", "status"):
            refused(entry, spaces(st, True), null=null)
    # the older entry points refuse what they refused: a streamed handle, and nfeat = 128 at create
    refused("ellhip_batch_svm_optim", spaces(False, True))
    refused("ellhip_batch_svm_optim_stable", spaces(True, True))
    with pytest.raises(gpu.capi.EllHipError, match="127"):
        gpu.BatchSvmProblem(np.zeros((2, 4, 128)), np.ones((2, 4), dtype=np.int32))
    with pytest.raises(gpu.capi.EllHipError, match="1023"):
        gpu.BatchSvmProblem.streamed(np.zeros((2, 4, 1024)), np.ones((2, 4), dtype=np.int32))
    assert prob.last()[1].tolist() == [INF] * B
    # and the good pairs still run
    for st in (False, True):
        recs = [ref.run(data[b], lab[b], 40, 1e-10, space=cpu_space(st, n)) for b in range(B)]
        check_loop(gpu, st, data, lab, recs, 40, 1e-10, prob=gpu.BatchSvmProblem.streamed(data, lab))


# ---- 9. the C++ mirror ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES)
def test_cpp_runner_matches_the_cpu_runs(gpu, tmp_path, stable):
    import cpp_build
    (m, nfeat, s), max_iters = pins.PINS[7][:2]   # (200, 129, 1), cut off at 40
    members = (s + 3, s, s + 6)
    data, lab = family_arrays(members, m, nfeat)
    path = tmp_path / "family.bin"
    path.write_bytes(struct.pack("<5qd", len(members), m, nfeat, max_iters, int(stable), TOL) + data.tobytes() +
                     lab.astype(np.int32).tobytes())
    exe = cpp_build.build_runner("batch_svm_streamed_runner.cpp", "hip")
    got = cpp_build.run_json_lines(exe, str(path))
    assert len(got) == len(members)
    hexbits = lambda v: format(int(np.float64(v).view(np.uint64)), "016x")
    for b, member in enumerate(members):
        d, r = got[f"sweep_{b}"], pins.record(stable, member, m, nfeat, max_iters)
        assert d["niter"] == r["niter"] and d["status"] == r["status"] and d["has_best"] == 1
        assert d["gamma"] == hexbits(r["gamma"]) and d["x_best"] == [hexbits(v) for v in r["x_best"]]
        assert d["min_idx"] == r["min_idx"] and d["min_val"] == hexbits(r["min_val"])
