"""GPU: the batched device-resident LMI loops on streamed batch handles (include/ellhip_batch_lmi_streamed.h), Ell and
EllStable, against the round-robin oracle of tests/batch_lmi_reference.py, its cutting_plane_optim / cutting_plane_feas over
the CPU oracle's spaces (tests/batch_lmi_streamed_cases.py) and the same loops on the LDS engine.  The device folds F(x), the
factorisation, the witness and the quadratic forms like the CPU, so every comparison is EXACT: float64 bit patterns (the
sign of a zero counts; NaN is compared by position) and integers -- gradient, beta, station, gamma, idx, x_best / x,
has_best / feasible, niter, status and the spaces' matrix (EllStable: the packed buffer, scratch triangle included), xc,
kappa and tsq afterwards.

The pinned counts are those of tests/test_batch_lmi_streamed_cpu.py; the cached records of the cases module are used here."""
import ctypes as C
import struct

import numpy as np
import pytest

import batch_lmi_reference as ref
import batch_lmi_streamed_cases as cases
import test_batch_lmi_streamed_cpu as pins
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INF = np.inf
SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]
LOOPS = [pytest.param(False, id="optim"), pytest.param(True, id="feas")]
SMALL = (129, (64, 3))   # the shape of the tests that are not about the shape


def same_bits(a, b):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def assert_bits(got, want, what):
    assert same_bits(got, want), (what, got, want)


def batch_class(gpu, stable, streamed=True):
    return {(False, True): gpu.EllBatchStreamed, (True, True): gpu.EllStableBatchStreamed,
            (False, False): gpu.EllBatch, (True, False): gpu.EllStableBatch}[(stable, streamed)]


def new_spaces(gpu, stable, kappa, xc, streamed=True):
    batch = batch_class(gpu, stable, streamed).new_with_scalar(np.array(kappa), np.array(xc))
    assert bool(getattr(batch, "is_streamed", False)) == streamed
    assert batch.variant == (gpu.capi.SPACE_ELL_STABLE if stable else gpu.capi.SPACE_ELL)
    return batch


def new_problem(gpu, mat_f, mat_b, c, feas, *, shared=False, streamed=True):
    """the pencils of `stack`; shared: problem 0's pencil for everyone"""
    c = None if feas else c
    if not streamed:
        return gpu.BatchLmiProblem(mat_f, mat_b, c)
    if shared:
        return gpu.BatchLmiProblem.streamed([f[0] for f in mat_f], mat_b, c, shared=True)
    return gpu.BatchLmiProblem.streamed(mat_f, mat_b, c)


def loop(prob, spaces, feas, max_iters, tol, gamma=INF):
    """-> (x, has, niter, status, gamma or None)"""
    if feas:
        x, ok, niter, status = prob.feas(spaces, max_iters, tol)
        return x, ok, niter, status, None
    x, has, niter, gamma, status = prob.optim(spaces, gamma, max_iters, tol)
    return x, has, niter, status, gamma


def assert_runs_equal(got, recs, n):
    x, has, niter, status, gamma = got
    np.testing.assert_array_equal(niter, np.array([r["niter"] for r in recs], dtype=np.int64))
    np.testing.assert_array_equal(status, np.array([r["status"] for r in recs], dtype=np.int32))
    np.testing.assert_array_equal(has, np.array([r["x"] is not None for r in recs], dtype=np.int32))
    if gamma is not None:
        assert_bits(gamma, np.array([r["gamma"] for r in recs]), "gamma")
    want = np.stack([np.full(n, np.nan) if r["x"] is None else r["x"] for r in recs])
    assert_bits(x, want, "x")   # rows without a result stay as the caller left them (NaN)


def assert_state_equal(prob, spaces, recs):
    np.testing.assert_array_equal(prob.idx, np.array([r["idx"] for r in recs], dtype=np.int32))
    assert_bits(spaces.mq, np.stack([r["mq"] for r in recs]), "mq")
    assert_bits(spaces.xc(), np.stack([r["xc"] for r in recs]), "xc")
    assert_bits(spaces.kappa, np.array([r["kappa"] for r in recs]), "kappa")
    assert_bits(spaces.tsq(), np.array([r["tsq"] for r in recs]), "tsq")


def check_loop(gpu, stable, feas, stacked, recs, max_iters, tol, *, chunk=None, spaces=None, prob=None, shared=False,
               gamma=INF):
    mat_f, mat_b, c, kappa, xc = stacked
    n = xc.shape[1]
    prob = new_problem(gpu, mat_f, mat_b, c, feas, shared=shared) if prob is None else prob
    if chunk is not None:
        prob.set_chunk(chunk)
    spaces = new_spaces(gpu, stable, kappa, xc) if spaces is None else spaces
    got = loop(prob, spaces, feas, max_iters, tol, gamma)
    assert_runs_equal(got, recs, n)
    assert_state_equal(prob, spaces, recs)
    return prob, spaces, got


def cpu_runs(stable, feas, n, ms, who, max_iters, tol, *, spaces=None, gammas=None, idx=None, shared=False, lmi0=False):
    """fresh CPU runs of the members (seed, t[, kf]); shared: problem who[0]'s pencil for everyone"""
    out = []
    for b, w in enumerate(who):
        fs, bs, c = cases.problem(w[0], n, ms)
        if shared:
            fs = cases.problem(who[0][0], n, ms)[0]
        space = cases.cpu_space(stable, *cases.start(w[0], n, ms, *w[1:])) if spaces is None else spaces[b]
        out.append(cases.run((fs, bs, c), space, feas=feas, max_iters=max_iters, tol=tol,
                             gamma=INF if gammas is None else gammas[b], idx=-1 if idx is None else idx[b], lmi0=lmi0))
    return out


# ---- 1. the oracle call by call ---------------------------------------------------------------------------------------------
# m = 1 (one element, 128 idle threads); m^2 > n with a tiny second block; m(m+1)/2 not a multiple of n; three blocks in a
# block of exactly 192 threads; n = 191 in 192 threads; the largest blocks, with and without inactive threads
CALL_SHAPES = [(129, (1,)), (129, (64, 3)), (130, (2, 63)), (192, (5, 17, 64)), (191, (64,)), (1023, (64,)), (1024, (64, 7)),
               (129, (1, 2, 3, 4, 5, 6, 7, 8))]
# (LMI0 form?, shared pencil?, with c?)
FORMS = [(False, False, True), (False, True, False), (True, False, False), (True, True, True)]


def oracle_call_by_call(gpu, n, ms):
    """three calls of the wide oracle kernel at (n; ms) in each of FORMS, with no update in between, against RoundRobinLmi"""
    B, J = 3, len(ms)
    who = [(s, 0.0) for s in range(B)]
    mat_f, mat_b, c, _, _ = cases.stack(n, ms, who)
    rng = np.random.default_rng(n + sum(ms))
    for lmi0, shared, with_c in FORMS:
        if lmi0:   # make x = e_0 strictly feasible for the homogeneous form, so that not every call is a cut
            mf = [f.copy() for f in mat_f]
            for f, m in zip(mf, ms):
                f[:, 0] += 3.0 * np.sqrt(n * m) * np.eye(m)
        else:
            mf = mat_f
        if shared:   # (mat_b or c tells the number of problems)
            prob = gpu.BatchLmiProblem.streamed([f[0] for f in mf], None if lmi0 else mat_b, c if with_c else None, shared=True)
        else:
            prob = gpu.BatchLmiProblem.streamed(mf, None if lmi0 else mat_b, c if with_c else None)
        assert prob.n == n and prob.J == J and prob.shared == shared
        omegas = [ref.RoundRobinLmi([(f[0] if shared else f[b]) for f in mf], None if lmi0 else [m_[b] for m_ in mat_b],
                                    c[b] if with_c else None) for b in range(B)]
        np.testing.assert_array_equal(prob.idx, np.full(B, -1, dtype=np.int32))
        gamma = np.full(B, INF)
        for call in range(3):
            if lmi0:   # near e_0 (feasible), then far from it
                x = 0.02 * rng.standard_normal((B, n)) * (1 + 40 * (call == 1))
                x[:, 0] += 1.0
            else:      # t h d with t around the boundary, a different t per problem and call
                x = np.stack([cases.start(s, n, ms, cases.T_VALUES[(s + 2 * call + 1) % 6])[1] for s in range(B)])
            grad, beta, station, gamma_out = prob.assess_optim(x, gamma)
            for b, om in enumerate(omegas):
                if with_c:
                    (g, bt), st, gm = om.assess_optim(x[b], gamma[b])
                else:
                    cut = om.assess_feas(x[b])
                    (g, bt), st, gm = ((np.zeros(n), 0.0), J + 1, gamma[b]) if cut is None else (cut[0], cut[1], gamma[b])
                assert station[b] == st, (lmi0, shared, with_c, call, b, station[b], st)
                assert_bits(grad[b], g, f"grad {call} {b}")
                assert same_bits(beta[b], bt) and same_bits(gamma_out[b], gm), (call, b, beta[b], bt, gamma_out[b], gm)
            np.testing.assert_array_equal(prob.idx, np.array([om.idx for om in omegas], dtype=np.int32))
            gamma = gamma_out


@pytest.mark.parametrize("n,ms", CALL_SHAPES, ids=["%d-%s" % (n, "x".join(map(str, ms))) for n, ms in CALL_SHAPES])
def test_oracle_call_by_call(gpu, n, ms):
    oracle_call_by_call(gpu, n, ms)


# ---- 2. the pinned runs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", pins.PIN_KEYS, ids=pins.PIN_IDS)
def test_pinned_runs(gpu, key):
    """every pinned batch: each run beside members that stop at other rounds"""
    bid, stable, feas = key
    n, ms, who, max_iters, tol, recs = cases.batch_records(bid, stable, feas)
    assert [(r["niter"], r["status"], r["x"] is not None, r["idx"]) for r in recs] == pins.PINS[key]
    check_loop(gpu, stable, feas, cases.stack(n, ms, who), recs, max_iters, tol)


# ---- 3. the reference's own problem and the LDS engine ----------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES)
def test_reference_problem(gpu, stable):
    """tests/lmi_tests.rs:174-185 on streamed handles: the CPU run and the LDS engine"""
    B, n = 4, 3
    fs, bs, c = ref.reference_problem()
    probs = [(fs, bs, c)] + [ref.family_a(s) for s in range(1, B)]
    mat_f, mat_b, cc = ref.stack(probs)
    kappa, xc = np.full(B, 10.0), np.zeros((B, n))
    for feas in (False, True):
        recs = [cases.run(p, cases.cpu_space(stable, 10.0, np.zeros(n)), feas=feas, max_iters=2000, tol=1e-8) for p in probs]
        if not feas:
            assert recs[0]["niter"] > 5 and recs[0]["x"] is not None
        prob, spaces, got = check_loop(gpu, stable, feas, (mat_f, mat_b, cc, kappa, xc), recs, 2000, 1e-8)
        lds_prob = new_problem(gpu, mat_f, mat_b, cc, feas, streamed=False)
        lds = new_spaces(gpu, stable, kappa, xc, streamed=False)
        want = loop(lds_prob, lds, feas, 2000, 1e-8)
        assert_runs_equal(want, recs, n)
        assert_state_equal(lds_prob, lds, recs)


# M small enough for the LDS engine to take the shape: M <= 8 at n = 128, and at n = 3, where a workgroup holds 64 problems
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("n,ms", [(2, (3, 2)), (3, (8,)), (64, (64, 5)), (65, (33, 8)), (128, (8, 7))])
def test_equals_the_lds_engine(gpu, stable, n, ms):
    """the same oracle data and the same start on both engines; an oracle handle of either constructor serves both"""
    who = [(0, 1.5), (1, 0.0), (2, 3.0), (0, 1.02)]
    stacked = cases.stack(n, ms, who)
    mat_f, mat_b, c, kappa, xc = stacked
    for feas in (False, True):
        recs = cpu_runs(stable, feas, n, ms, who, 30, 0.0)
        lds_prob = new_problem(gpu, mat_f, mat_b, c, feas, streamed=False)
        lds = new_spaces(gpu, stable, kappa, xc, streamed=False)
        want = loop(lds_prob, lds, feas, 30, 0.0)
        assert_runs_equal(want, recs, n)
        assert_state_equal(lds_prob, lds, recs)
        for streamed_ctor in (True, False):
            prob = new_problem(gpu, mat_f, mat_b, c, feas, streamed=streamed_ctor)
            spaces = new_spaces(gpu, stable, kappa, xc)
            got = loop(prob, spaces, feas, 30, 0.0)
            for g, w, what in zip(got, want, ("x", "has", "niter", "status", "gamma")):
                if g is None:
                    assert w is None
                elif g.dtype == np.float64:
                    assert_bits(g, w, what)
                else:
                    np.testing.assert_array_equal(g, w, err_msg=what)
            np.testing.assert_array_equal(prob.idx, lds_prob.idx)
            for g, w, what in ((spaces.mq, lds.mq, "mq"), (spaces.xc(), lds.xc(), "xc"), (spaces.kappa, lds.kappa, "kappa"),
                               (spaces.tsq(), lds.tsq(), "tsq")):
                assert_bits(g, w, what)
        # a streamed-constructor handle on the LDS engine
        again = new_spaces(gpu, stable, kappa, xc, streamed=False)
        prob = new_problem(gpu, mat_f, mat_b, c, feas)
        assert_runs_equal(loop(prob, again, feas, 30, 0.0), recs, n)
        assert_state_equal(prob, again, recs)


# ---- 4. launches, stops and what lies between two calls ---------------------------------------------------------------------
WHO = cases.members(SMALL[0])


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("feas", LOOPS)
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunking_changes_nothing(gpu, stable, feas, chunk):
    """chunk 1: the early oracle call is never made and no sweep is fused; 7: six fused rounds, then a plain one; 256: one
    launch"""
    n, ms, who, max_iters, tol, recs = cases.batch_records("129-64x3", stable, feas)
    check_loop(gpu, stable, feas, cases.stack(n, ms, who), recs, max_iters, tol, chunk=chunk)


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("feas", LOOPS)
def test_cut_off_and_resume(gpu, stable, feas):
    """cut off at round 11 and resumed by a second call: idx and gamma carry over, and the whole equals one call"""
    n, ms = SMALL
    stacked = cases.stack(n, ms, WHO)
    spaces_cpu = [cases.cpu_space(stable, *cases.start(s, n, ms, t)) for s, t in WHO]
    first = cpu_runs(stable, feas, n, ms, WHO, 11, 0.0, spaces=spaces_cpu)
    prob, spaces, got = check_loop(gpu, stable, feas, stacked, first, 11, 0.0)
    gammas = None if feas else [r["gamma"] for r in first]
    second = cpu_runs(stable, feas, n, ms, WHO, 19, 0.0, spaces=spaces_cpu, gammas=gammas, idx=[r["idx"] for r in first])
    whole = cases.batch_records("129-64x3", stable, feas)[-1]
    for f, s, w in zip(first, second, whole):
        if f["niter"] == 11 and not (feas and f["x"] is not None):   # cut off, not ended: the two calls make the one run
            assert f["niter"] + s["niter"] == w["niter"] and same_bits(s["mq"], w["mq"]) and s["idx"] == w["idx"]
    got2 = loop(prob, spaces, feas, 19, 0.0, INF if feas else got[4])
    assert_runs_equal(got2, second, n)
    assert_state_equal(prob, spaces, second)


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("feas", LOOPS)
def test_max_iters_zero_moves_nothing(gpu, stable, feas):
    n, ms = SMALL
    first = cpu_runs(stable, feas, n, ms, WHO, 9, 0.0)
    prob, spaces, got = check_loop(gpu, stable, feas, cases.stack(n, ms, WHO), first, 9, 0.0)
    x, has, niter, status, gamma = loop(prob, spaces, feas, 0, 0.0, INF if feas else got[4])
    assert not has.any() and not niter.any() and not status.any() and np.isnan(x).all()
    if not feas:
        assert_bits(gamma, got[4], "gamma")
    assert_state_equal(prob, spaces, first)


@pytest.mark.parametrize("stable", SPACES)
def test_set_idx_between_two_loops(gpu, stable):
    n, ms = SMALL
    J = len(ms)
    spaces_cpu = [cases.cpu_space(stable, *cases.start(s, n, ms, t)) for s, t in WHO]
    first = cpu_runs(stable, False, n, ms, WHO, 7, 0.0, spaces=spaces_cpu)
    prob, spaces, got = check_loop(gpu, stable, False, cases.stack(n, ms, WHO), first, 7, 0.0)
    idx = np.array([J, -1, 0, 1, J, 0], dtype=np.int32)
    assert not np.array_equal(idx, prob.idx)
    prob.idx = idx
    second = cpu_runs(stable, False, n, ms, WHO, 12, 0.0, spaces=spaces_cpu, gammas=[r["gamma"] for r in first], idx=idx.tolist())
    assert_runs_equal(loop(prob, spaces, False, 12, 0.0, got[4]), second, n)
    assert_state_equal(prob, spaces, second)
    prob.idx = None
    np.testing.assert_array_equal(prob.idx, np.full(len(WHO), -1, dtype=np.int32))
    with pytest.raises(gpu.capi.EllHipError):
        prob.idx = np.full(len(WHO), J + 1, dtype=np.int32)


@pytest.mark.parametrize("stable", SPACES)
def test_batch_update_between_two_loops(gpu, stable):
    n, ms = SMALL
    B = len(WHO)
    spaces_cpu = [cases.cpu_space(stable, *cases.start(s, n, ms, t)) for s, t in WHO]
    first = cpu_runs(stable, False, n, ms, WHO, 10, 0.0, spaces=spaces_cpu)
    prob, spaces, got = check_loop(gpu, stable, False, cases.stack(n, ms, WHO), first, 10, 0.0)
    rng = np.random.default_rng(3)
    grads = rng.standard_normal((1, B, n))
    kinds = rng.integers(0, 2, size=(1, B)).astype(np.int32)
    beta = np.zeros((1, B))
    want = np.zeros((1, B), dtype=np.int32)
    for b, space in enumerate(spaces_cpu):
        beta[0, b] = 0.1 * np.sqrt(space.tsq) if kinds[0, b] == 0 else 0.0
        want[0, b] = space.update(int(kinds[0, b]), grads[0, b], beta[0, b])
    status, _ = spaces.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    after = [dict(first[b], **cases.space_record(spaces_cpu[b])) for b in range(B)]
    assert_state_equal(prob, spaces, after)
    second = cpu_runs(stable, False, n, ms, WHO, 15, 0.0, spaces=spaces_cpu, gammas=[r["gamma"] for r in first],
                      idx=[r["idx"] for r in first])
    assert_runs_equal(loop(prob, spaces, False, 15, 0.0, got[4]), second, n)
    assert_state_equal(prob, spaces, second)


@pytest.mark.parametrize("stable", SPACES)
def test_from_space_clone(gpu, stable):
    """one start for every problem: a clone of a single space"""
    n, ms = SMALL
    who = [(0, 1.5), (1, 1.5), (2, 1.5)]
    kappa, xc = cases.start(0, n, ms, 1.5)
    mat_f, mat_b, c, _, _ = cases.stack(n, ms, who)
    recs = [cases.run(cases.problem(s, n, ms), cases.cpu_space(stable, kappa, xc), feas=False, max_iters=20, tol=0.0)
            for s, _ in who]
    if stable:
        spaces = gpu.EllStableBatchStreamed.from_space(gpu.EllStable.new_with_scalar(kappa, xc), len(who))
    else:
        spaces = gpu.EllBatchStreamed.from_space(gpu.Ell.new_with_scalar(kappa, xc), len(who))
    assert spaces.is_streamed
    stacked = (mat_f, mat_b, c, np.full(len(who), kappa), np.tile(xc, (len(who), 1)))
    check_loop(gpu, stable, False, stacked, recs, 20, 0.0, spaces=spaces)


def test_no_defer_trick(gpu):
    n, ms = SMALL
    stacked = cases.stack(n, ms, WHO)
    spaces = new_spaces(gpu, False, stacked[3], stacked[4])
    spaces.set_no_defer_trick(True)
    spaces_cpu = [cases.cpu_space(False, *cases.start(s, n, ms, t)) for s, t in WHO]
    for space in spaces_cpu:
        space.set_no_defer_trick(True)
    recs = cpu_runs(False, False, n, ms, WHO, 30, 0.0, spaces=spaces_cpu)
    plain = cases.batch_records("129-64x3", False, False)[-1]
    assert not np.array_equal(recs[3]["mq"], plain[3]["mq"])   # the flag does something
    check_loop(gpu, False, False, stacked, recs, 30, 0.0, spaces=spaces)


def test_non_symmetric_start(gpu):
    """Ell, n = 129: the first round takes the mirror sweep (the product by rows), later ones the fused sweep"""
    n, ms = SMALL
    B = len(WHO)
    mat_f, mat_b, c, kappa, xc = cases.stack(n, ms, WHO)
    rng = np.random.default_rng(219)
    mq = np.stack([np.eye(n) * (1.0 + rng.random()) + (0.1 / n) * rng.standard_normal((n, n)) for _ in range(B)])
    assert not np.array_equal(mq, np.swapaxes(mq, 1, 2))
    for max_iters in (30, 1):   # (one round only: the mirror sweep alone)
        spaces = gpu.EllBatchStreamed.new_with_matrix(kappa, mq, xc)
        spaces_cpu = [O.OracleEll.new_with_matrix(kappa[b], mq[b], xc[b]) for b in range(B)]
        recs = cpu_runs(False, False, n, ms, WHO, max_iters, 0.0, spaces=spaces_cpu)
        check_loop(gpu, False, False, (mat_f, mat_b, c, kappa, xc), recs, max_iters, 0.0, spaces=spaces)
        if max_iters == 30:
            q = spaces.mq
            assert_bits(q, np.swapaxes(q, 1, 2), "mirrored")


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("feas", LOOPS)
def test_shared_pencil_equals_the_pencil_given_b_times(gpu, stable, feas):
    """one pencil, B different B_j, c and starts: shared_f = 1 against the same pencil stacked B times, and the CPU"""
    n, ms = SMALL
    mat_f, mat_b, c, kappa, xc = cases.stack(n, ms, WHO)
    tiled = [np.broadcast_to(f[0], f.shape).copy() for f in mat_f]
    recs = cpu_runs(stable, feas, n, ms, WHO, 30, 0.0, shared=True)
    assert len({r["niter"] for r in recs}) > 1 or not feas
    a = check_loop(gpu, stable, feas, (mat_f, mat_b, c, kappa, xc), recs, 30, 0.0, shared=True)
    b = check_loop(gpu, stable, feas, (tiled, mat_b, c, kappa, xc), recs, 30, 0.0)
    assert a[0].shared and not b[0].shared
    for g, w in zip(a[2], b[2]):
        assert (g is None and w is None) or same_bits(g.astype(np.float64), w.astype(np.float64))
    assert_bits(a[1].mq, b[1].mq, "mq")


# ---- 5. more workgroups than the card holds at once -------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-problem"])
def test_large_population(gpu, shared):
    """B = 600 at (129; 8, 5), 6 rounds: twelve different members, each fifty times"""
    n, ms, distinct, B, max_iters = 129, (8, 5), 12, 600, 6
    who = [(i % 4, cases.T_VALUES[(i * 5 + 1) % 6]) for i in range(distinct)]
    mat_f, mat_b, c, kappa, xc = cases.stack(n, ms, who)
    recs = cpu_runs(False, False, n, ms, who, max_iters, 0.0, shared=shared)
    assert len({r["stations"] for r in recs}) > 3
    reps = B // distinct
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))
    stacked = ([tile(f) for f in mat_f], [tile(m_) for m_ in mat_b], tile(c), tile(kappa), tile(xc))
    check_loop(gpu, False, False, stacked, recs * reps, max_iters, 0.0, shared=shared)


# ---- 6. above 64 KiB of LDS -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES)
def test_above_64_kib_of_lds(gpu, stable):
    """n = 1024, M = 64: 89.2 KiB (Ell) and 81.7 KiB (EllStable) of LDS.  On Ell the same shape on two handles in turn: the
    opt-in is taken once and reused; then a smaller shape, which must not lower it, and the first again"""
    n, ms, who, max_iters, tol, recs = cases.batch_records("1024-64x7", stable, False)
    keep = [3, 4, 5]   # the three members that cut at blocks
    stacked = tuple(([f[keep] for f in part] if isinstance(part, list) else part[keep]) for part in cases.stack(n, ms, who))
    sub = [recs[k] for k in keep]
    prob, _, _ = check_loop(gpu, stable, False, stacked, sub, max_iters, tol)
    if stable:
        return
    prob.idx = None
    check_loop(gpu, stable, False, stacked, sub, max_iters, tol, prob=prob)
    check_loop(gpu, stable, False, stacked, sub, max_iters, tol)
    small = cases.batch_records("129-64x3", False, False)
    check_loop(gpu, False, False, cases.stack(*small[:3]), small[-1], small[3], small[4])
    check_loop(gpu, stable, False, stacked, sub, max_iters, tol)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(gpu):
    lib = gpu.capi.load()
    n, ms, B = 64, (5, 3), 3
    who = [(s, 1.5) for s in range(B)]
    mat_f, mat_b, c, kappa, xc = cases.stack(n, ms, who)
    with_c = gpu.BatchLmiProblem.streamed(mat_f, mat_b, c)
    without_c = gpu.BatchLmiProblem.streamed(mat_f, mat_b)
    for prob in (with_c, without_c):
        prob.idx = np.array([1, 0, -1], dtype=np.int32)
    rng = np.random.default_rng(2)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def refused(entry, spaces, oracle, null=None):
        feas = "_feas" in entry
        before = (spaces.mq, spaces.xc(), spaces.kappa, spaces.tsq())
        idx = oracle.idx
        gamma = np.full(spaces.B, 0.3)
        x = np.full((spaces.B, spaces.n), np.nan)
        has = np.full(spaces.B, -5, dtype=np.int32)
        niter = np.full(spaces.B, -5, dtype=np.int64)
        status = np.full(spaces.B, -5, dtype=np.int32)
        args = dict(gamma=gamma, has=has, niter=niter, status=status)
        if null is not None:
            args[null] = None
        head = (spaces._h if null != "spaces" else None, oracle._h if null != "oracle" else None)
        head += () if feas else (ptr(args["gamma"]),)
        rc = getattr(lib, entry)(*head, 100, 1e-10, ptr(x), ptr(args["has"]), ptr(args["niter"]), ptr(args["status"]))
        assert rc == gpu.capi.E_INVALID and lib.ellhip_last_error(), (entry, null)
        for a, b in zip(before, (spaces.mq, spaces.xc(), spaces.kappa, spaces.tsq())):
            assert same_bits(a, b)
        np.testing.assert_array_equal(oracle.idx, idx)
        assert np.isnan(x).all() and (gamma == 0.3).all()
        assert (has == -5).all() and (niter == -5).all() and (status == -5).all()

    def spaces(stable, streamed, B=B, n=n):
        return batch_class(gpu, stable, streamed).new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n)))

    for kind, oracle, other in (("optim", with_c, without_c), ("feas", without_c, with_c)):
        ell, stable = f"ellhip_batch_lmi_{kind}_streamed", f"ellhip_batch_lmi_{kind}_streamed_stable"
        refused(ell, spaces(False, False), oracle)            # LDS handles
        refused(ell, spaces(True, False), oracle)
        refused(stable, spaces(True, False), oracle)
        refused(stable, spaces(False, False), oracle)
        refused(ell, spaces(True, True), oracle)              # the other variant
        refused(stable, spaces(False, True), oracle)
        for entry, st in ((ell, False), (stable, True)):
            refused(entry, spaces(st, True, B=B + 1), oracle)     # B
            refused(entry, spaces(st, True, n=n + 1), oracle)     # n
            refused(entry, spaces(st, True), other)               # optim without c, feas with c
            nulls = ("spaces", "oracle", "has", "niter", "status") + (() if kind == "feas" else ("gamma",))
            for null in nulls:
                refused(entry, spaces(st, True), oracle, null=null)
        # the older entry points refuse what they refused: streamed handles
        refused(f"ellhip_batch_lmi_{kind}", spaces(False, True), oracle)
        refused(f"ellhip_batch_lmi_{kind}_stable", spaces(True, True), oracle)
    # and the old constructor stops at n = 128
    with pytest.raises(gpu.capi.EllHipError, match="128"):
        gpu.BatchLmiProblem([np.zeros((2, 129, 2, 2))], c=np.zeros((2, 129)))
    with pytest.raises(gpu.capi.EllHipError, match="1024"):
        gpu.BatchLmiProblem.streamed([np.zeros((2, 1025, 2, 2))], c=np.zeros((2, 1025)))
    # the good pairs still run
    for st in (False, True):
        for feas, prob in ((False, with_c), (True, without_c)):
            prob.idx = None
            recs = cpu_runs(st, feas, n, ms, who, 25, 0.0)
            check_loop(gpu, st, feas, (mat_f, mat_b, c, kappa, xc), recs, 25, 0.0, prob=prob)


# ---- 8. the C++ mirror ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable,feas,shared", [(False, False, False), (True, True, False), (False, True, True)],
                         ids=["ell-optim", "stable-feas", "ell-feas-shared"])
def test_cpp_runner_matches_the_cpu_runs(gpu, tmp_path, stable, feas, shared):
    import cpp_build
    n, ms, who, max_iters, tol, recs = cases.batch_records("129-64x3", stable, feas)
    if shared:
        recs = cpu_runs(stable, feas, n, ms, who, max_iters, tol, shared=True)
    mat_f, mat_b, c, kappa, xc = cases.stack(n, ms, who)
    blob = struct.pack("<7q", len(who), n, len(ms), max_iters, int(stable), int(feas), int(shared))
    blob += struct.pack("<%dq" % len(ms), *ms) + struct.pack("<d", tol) + kappa.tobytes() + xc.tobytes() + c.tobytes()
    for f, m_ in zip(mat_f, mat_b):
        blob += (f[0] if shared else f).tobytes() + m_.tobytes()
    path = tmp_path / "family.bin"
    path.write_bytes(blob)
    exe = cpp_build.build_runner("batch_lmi_streamed_runner.cpp", "hip")
    got = cpp_build.run_json_lines(exe, str(path))
    assert len(got) == len(who)
    hexbits = lambda v: format(int(np.float64(v).view(np.uint64)), "016x")
    for b, r in enumerate(recs):
        d = got[f"sweep_{b}"]
        assert d["niter"] == r["niter"] and d["status"] == r["status"] and d["has_x"] == int(r["x"] is not None)
        assert d["idx"] == r["idx"] and d["x"] == ([] if r["x"] is None else [hexbits(v) for v in r["x"]])
        if not feas:
            assert d["gamma"] == hexbits(r["gamma"])
