"""GPU: the batched device-resident bsearch (include/ellhip_batch_bsearch.h) against the CPU restatement
(tests/batch_bsearch_reference.py), in every bit: the reference's pin, the seeded family at every launch shape of the LDS
engines, launch boundaries inside probes, a second call on the same handles, the degenerate options, the host-driven form
built from the _feas entry point, no_defer_trick, J = 1, shared against per-problem tables, the oracle alone, and the
refusals."""
import numpy as np
import pytest

import batch_bsearch_reference as ref

pytestmark = pytest.mark.gpu

WIDE, SHORT = (2000, 1e-8), (25, 1e-8)
SHAPES = [  # (n, B, inner, outer)
    (2, 200, WIDE, ref.OUTER), (2, 200, SHORT, ref.OUTER), (2, 1, WIDE, ref.OUTER), (2, 1, SHORT, ref.OUTER),
    (2, 65, WIDE, ref.OUTER), (2, 65, SHORT, ref.OUTER), (3, 70, WIDE, ref.OUTER), (3, 70, SHORT, ref.OUTER),
    (5, 52, WIDE, ref.OUTER), (5, 52, SHORT, ref.OUTER), (16, 17, (40, 1e-8), ref.OUTER), (33, 7, (40, 1e-8), (12, 1e-8)),
    (64, 5, (30, 1e-8), (6, 1e-8)), (65, 2, (30, 1e-8), (6, 1e-8)), (128, 2, (30, 1e-8), (6, 1e-8)),
]
SPACES = [False, True]
IDS = ["ell", "stable"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64 or b.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and np.array_equal(a, b)


def make(gpu, n, B, stable, *, shared_member=None, no_defer_trick=False):
    """(batch, problem) for the first B members (or B copies of one member behind one shared table)"""
    a, c, xc0 = ref.tables(n, B)
    cls = gpu.EllStableBatch if stable else gpu.EllBatch
    if shared_member is not None:
        a1, c1, x1 = ref.family(shared_member, n)
        batch = cls.new_with_scalar(ref.KAPPA, np.tile(x1, (B, 1)))
        prob = gpu.BatchLinFeasProblem(a1, c1, B)
    else:
        batch = cls.new_with_scalar(ref.KAPPA, xc0)
        prob = gpu.BatchLinFeasProblem(a, c)
    if no_defer_trick:
        batch.set_no_defer_trick(True)
    return batch, prob


def snapshot(batch):
    return batch.mq.copy(), batch.kappa.copy(), batch.tsq().copy(), batch.xc().copy()


def check_run(batch, prob, got, want, before):
    feasible, niter, upper, rounds, ends = got
    assert same(feasible, want["feasible"])
    assert same(niter, want["niter"])
    assert same(upper, want["upper"])
    assert same(rounds, want["rounds"])
    assert same(ends, want["ends"])
    idx, target = prob.state()
    assert same(idx, want["idx"]) and same(target, want["target"])
    assert same(batch.xc(), want["xc"])
    assert same(batch.mq, before[0]) and same(batch.kappa, before[1]) and same(batch.tsq(), before[2])


# ---- the pin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_pin(gpu, stable):
    want = ref.pin(stable)
    assert want["feasible"] and want["niter"] == 34                                    # src/example3.rs:82-84
    cls = gpu.EllStableBatch if stable else gpu.EllBatch
    batch = cls.new_with_scalar(100.0, np.zeros((1, 2)))
    prob = gpu.BatchLinFeasProblem(np.array(ref.EX3_A), np.array(ref.EX3_C), 1)
    before = snapshot(batch)
    got = prob.bsearch(batch, -100.0, 100.0, 2000, 1e-8, 2000, 1e-8)
    one = {k: np.array([want[k]]) for k in ("feasible", "niter", "upper", "rounds", "idx", "target")}
    one["ends"], one["xc"] = np.array([want["ends"]]), want["xc"][None]
    check_run(batch, prob, got, one, before)


# ---- the family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES, ids=IDS)
@pytest.mark.parametrize("n,B,inner,outer", SHAPES, ids=[f"n{s[0]}-B{s[1]}-inner{s[2][0]}" for s in SHAPES])
def test_family(gpu, n, B, inner, outer, stable):
    want = ref.runs(n, B, stable, inner, outer)
    batch, prob = make(gpu, n, B, stable)
    before = snapshot(batch)
    got = prob.bsearch(batch, *ref.INTERVAL, *inner, *outer)
    check_run(batch, prob, got, want, before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunks(gpu, chunk, stable):
    """chunk 1 puts a launch boundary inside every probe"""
    n, B = 2, 65
    for inner in (WIDE, SHORT):
        want = ref.runs(n, B, stable, inner)
        batch, prob = make(gpu, n, B, stable)
        prob.set_chunk(chunk)
        before = snapshot(batch)
        check_run(batch, prob, prob.bsearch(batch, *ref.INTERVAL, *inner, *ref.OUTER), want, before)
    n, B, inner, outer = 33, 7, (40, 1e-8), (12, 1e-8)
    want = ref.runs(n, B, stable, inner, outer)
    batch, prob = make(gpu, n, B, stable)
    prob.set_chunk(chunk)
    before = snapshot(batch)
    check_run(batch, prob, prob.bsearch(batch, *ref.INTERVAL, *inner, *outer), want, before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_second_call_continues(gpu, stable):
    n, B, half = 3, 70, 0.125
    first, want = ref.runs(n, B, stable, WIDE), ref.runs(n, B, stable, WIDE, again=half)
    batch, prob = make(gpu, n, B, stable)
    before = snapshot(batch)
    got = prob.bsearch(batch, *ref.INTERVAL, *WIDE, *ref.OUTER)
    check_run(batch, prob, got, first, before)
    check_run(batch, prob, prob.bsearch(batch, got[2] - half, got[2] + half, *WIDE, *ref.OUTER), want, before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_degenerate_options(gpu, stable):
    n, B = 2, 65
    batch, prob = make(gpu, n, B, stable)
    before = snapshot(batch)
    lo, up = ref.INTERVAL
    idle = {"feasible": np.zeros(B, bool), "niter": np.zeros(B, np.int64), "upper": np.full(B, up),
            "rounds": np.zeros(B, np.int64), "ends": np.zeros((B, 4), np.int64), "idx": np.full(B, -1, np.int32),
            "target": np.full(B, -1e100), "xc": before[3]}
    check_run(batch, prob, prob.bsearch(batch, lo, up, *WIDE, 0, 1e-8), idle, before)            # max_iters = 0
    check_run(batch, prob, prob.bsearch(batch, lo, up, *WIDE, 2000, 51.0), idle, before)         # the first tau < tol
    check_run(batch, prob, prob.bsearch(batch, 3.0, 3.0, *WIDE, 2000, 1e-8),                     # lower == upper
              dict(idle, upper=np.full(B, 3.0)), before)
    want = ref.runs(n, B, stable, WIDE, (1, 1e-8))                                               # max_iters = 1
    assert set(want["niter"]) == {1}
    check_run(batch, prob, prob.bsearch(batch, lo, up, *WIDE, 1, 1e-8), want, before)
    # inner_max_iters = 0: every probe ends without an oracle call, the target moves
    batch, prob = make(gpu, n, B, stable)
    want = ref.runs(n, B, stable, (0, 1e-8), (5, 1e-8))
    assert not want["feasible"].any() and (want["ends"][:, 3] == 5).all() and (want["rounds"] == 0).all()
    check_run(batch, prob, prob.bsearch(batch, lo, up, 0, 1e-8, 5, 1e-8), want, before)


# ---- the host-driven form: what a user has with _feas alone -------------------------------------------------------------------
def host_driven(gpu, batch, prob, lower, upper, inner, outer):
    """bsearch in numpy; each probe is a fresh batch handle built from the getters, then set_target, feas, set_xc"""
    B = batch.B
    cls = type(batch)
    lower, upper = np.full(B, lower), np.full(B, upper)
    u_orig = upper.copy()
    rounds = np.zeros(B, np.int64)
    niter_out = outer[0]
    for niter in range(outer[0]):
        tau = (upper - lower) / 2.0
        stop = tau < outer[1]
        assert stop.all() or not stop.any()        # (the family's intervals stay as wide as each other)
        if stop.all():
            niter_out = niter
            break
        gamma = lower + tau
        probe = cls.new_with_matrix(batch.kappa, batch.mq, batch.xc())
        prob.set_target(gamma)
        x, has, k, _ = prob.feas(probe, *inner)
        has = has.astype(bool)
        rounds += k + (k < inner[0])
        batch.set_xc(np.where(has[:, None], x, batch.xc()))
        upper = np.where(has, gamma, upper)
        lower = np.where(has, lower, gamma)
    return upper != u_orig, np.full(B, niter_out, np.int64), upper, rounds


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_host_driven_form_agrees(gpu, stable):
    n, B, inner = 5, 52, SHORT
    want = ref.runs(n, B, stable, inner)
    batch, prob = make(gpu, n, B, stable)
    before = snapshot(batch)
    feasible, niter, upper, rounds = host_driven(gpu, batch, prob, *ref.INTERVAL, inner, ref.OUTER)
    check_run(batch, prob, (feasible, niter, upper, rounds, want["ends"]), want, before)


# ---- variations ---------------------------------------------------------------------------------------------------------------
def test_no_defer_trick(gpu):
    n, B = 3, 70
    want = ref.runs(n, B, False, WIDE, no_defer_trick=True)
    plain = ref.runs(n, B, False, WIDE)
    assert not same(want["xc"], plain["xc"])                   # the flag is seen: the clones' roundings differ
    batch, prob = make(gpu, n, B, False, no_defer_trick=True)
    before = snapshot(batch)
    check_run(batch, prob, prob.bsearch(batch, *ref.INTERVAL, *WIDE, *ref.OUTER), want, before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_one_row(gpu, stable):
    """J = 1: the only row is the target's"""
    n, B = 3, 9
    rng = np.random.default_rng(5)
    a, xc0 = rng.standard_normal((B, 1, n)), rng.uniform(-0.2, 0.2, (B, n))
    cls = gpu.EllStableBatch if stable else gpu.EllBatch
    batch, prob = cls.new_with_scalar(ref.KAPPA, xc0), gpu.BatchLinFeasProblem(a, np.zeros((B, 1)))
    before = snapshot(batch)
    got = prob.bsearch(batch, *ref.INTERVAL, *SHORT, *ref.OUTER)
    want = []
    for b in range(B):
        omega, space = ref.LinFeas(a[b], [0.0]), ref.space_of(stable, xc0[b])
        want.append(ref._record(omega, space, ref.bsearch(omega, space, *ref.INTERVAL, SHORT, ref.OUTER)))
    stacked = {k: np.array([w[k] for w in want]) for k in ("feasible", "niter", "upper", "rounds", "ends", "target", "xc")}
    stacked["idx"] = np.array([w["idx"] for w in want], dtype=np.int32)
    assert stacked["feasible"].all() and (stacked["idx"] == 0).all()
    check_run(batch, prob, got, stacked, before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_shared_table_equals_per_problem_tables(gpu, stable):
    n, B, member = 5, 52, 3
    a1, c1, x1 = ref.family(member, n)
    one = ref.run(member, n, stable, SHORT)
    cls = gpu.EllStableBatch if stable else gpu.EllBatch
    results = []
    for per_problem in (False, True):
        batch = cls.new_with_scalar(ref.KAPPA, np.tile(x1, (B, 1)))
        prob = gpu.BatchLinFeasProblem(np.tile(a1, (B, 1, 1)), np.tile(c1, (B, 1))) if per_problem else \
            gpu.BatchLinFeasProblem(a1, c1, B)
        results.append(prob.bsearch(batch, *ref.INTERVAL, *SHORT, *ref.OUTER) + prob.state() + (batch.xc(),))
    for u, v in zip(*results):
        assert same(u, v)
    assert same(results[0][2], np.full(B, one["upper"])) and same(results[0][3], np.full(B, one["rounds"], np.int64))


@pytest.mark.parametrize("n,B", [(2, 200), (5, 52), (33, 7), (128, 2)])
def test_assess_feas(gpu, n, B):
    a, c, xc0 = ref.tables(n, B)
    prob = gpu.BatchLinFeasProblem(a, c)
    omegas = [ref.LinFeas(a[b], c[b]) for b in range(B)]
    rng = np.random.default_rng(17)
    for call in range(6):
        if call == 3:
            gamma = rng.uniform(-3.0, 3.0, B)
            prob.set_target(gamma)
            for b in range(B):
                omegas[b].update(float(gamma[b]))
        x = rng.uniform(-4.0, 4.0, (B, n)) * (0.05 if call % 2 else 1.0)
        grad, beta, cut = prob.assess_feas(x)
        for b in range(B):
            w = omegas[b].assess_feas(x[b])
            if w is None:
                assert cut[b] == -1 and beta[b] == 0.0 and not grad[b].any()
            else:
                assert cut[b] == omegas[b].idx and same(grad[b], w[0]) and same(beta[b:b + 1], np.array([w[1]]))
        idx, target = prob.state()
        assert same(idx, np.array([o.idx for o in omegas], np.int32)) and same(target, np.array([o.target for o in omegas]))
    assert (cut == -1).any() or n > 5


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
@pytest.mark.parametrize("n,B", [(2, 65), (16, 17)])
def test_feas(gpu, n, B, stable):
    a, c, xc0 = ref.tables(n, B)
    batch, prob = make(gpu, n, B, stable)
    gamma = np.linspace(-20.0, 4.0, B)     # (n = 2: 18 feasible, 47 NoSoln; n = 16: 16 feasible, one at max_iters)
    prob.set_target(gamma)
    x, has, niter, status = prob.feas(batch, 60, 1e-8)
    ends = set()
    for b in range(B):
        omega, space = ref.LinFeas(a[b], c[b]), ref.space_of(stable, xc0[b])
        omega.update(float(gamma[b]))
        wx, wk, _, end = ref.cutting_plane_feas(omega, space, 60, 1e-8)
        ends.add(end)
        assert bool(has[b]) == (wx is not None) and niter[b] == wk
        if wx is not None:
            assert same(x[b], wx)
        assert same(batch.xc()[b], np.array(space.xc)) and same(batch.mq[b], np.array(space.mq))
    assert ref.END_FEASIBLE in ends and len(ends) > 1
    idx, target = prob.state()
    assert same(target, gamma)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(gpu):
    n, B = 2, 9
    a, c, xc0 = ref.tables(n, B)
    prob = gpu.BatchLinFeasProblem(a, c)
    ell, stable = gpu.EllBatch.new_with_scalar(ref.KAPPA, xc0), gpu.EllStableBatch.new_with_scalar(ref.KAPPA, xc0)
    streamed = gpu.EllBatchStreamed.new_with_scalar(ref.KAPPA, xc0)
    lib, E = prob._lib, gpu.capi.E_INVALID

    def call(entry, batch, problem, lower=-50.0, upper=50.0):
        lo, up = np.full(problem.B, lower), np.full(problem.B, upper)
        out = [np.full(problem.B, 7, np.int32), np.full(problem.B, 7, np.int64), np.full(problem.B, 7.0),
               np.full(problem.B, 7, np.int64), np.full((problem.B, 4), 7, np.int64)]
        before = snapshot(batch), problem.state()
        rc = getattr(lib, entry)(batch._h, problem._h, lo.ctypes.data, up.ctypes.data, 25, 1e-8, 2000, 1e-8,
                                 *[o.ctypes.data for o in out])
        assert rc == E and lib.ellhip_last_error()
        assert all((o == 7).all() for o in out)
        after = snapshot(batch), problem.state()
        for u, v in zip(before[0] + before[1], after[0] + after[1]):
            assert same(u, v)
        return lib.ellhip_last_error()

    plain, st = "ellhip_batch_linfeas_bsearch", "ellhip_batch_linfeas_bsearch_stable"
    assert b"not built" in call(plain, streamed, prob)
    call(st, streamed, prob)
    call(plain, stable, prob)                                   # the other variant
    call(st, ell, prob)
    other_b = gpu.BatchLinFeasProblem(*ref.tables(n, B + 1)[:2])
    call(plain, ell, other_b)                                   # B
    other_n = gpu.BatchLinFeasProblem(*ref.tables(3, B)[:2])
    call(plain, ell, other_n)                                   # n
    call(plain, ell, prob, lower=1.0, upper=0.5)                # lower > upper
    call(st, stable, prob, lower=1.0, upper=0.5)
    if lib.ellhip_device_count() > 1:
        far = gpu.BatchLinFeasProblem(a, c, device=1)
        call(plain, ell, far)
    with pytest.raises(gpu.capi.EllHipError):
        prob.feas(streamed, 10, 1e-8)
    with pytest.raises(gpu.capi.EllHipError):
        prob.bsearch(stable, 1.0, 0.0, 25, 1e-8, 10, 1e-8)
    # and the handles still work
    want = ref.runs(n, B, False, SHORT)
    before = snapshot(ell)
    check_run(ell, prob, prob.bsearch(ell, *ref.INTERVAL, *SHORT, *ref.OUTER), want, before)
