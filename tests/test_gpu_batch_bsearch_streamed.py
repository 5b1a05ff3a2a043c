"""GPU: the batched linear feasibility loops and the device-resident bsearch on streamed batch handles
(include/ellhip_batch_bsearch_streamed.h) against the CPU restatement (tests/batch_bsearch_reference.py), in every bit and on
both spaces: the reference's pin, the seeded family from n = 2 to n = 1024 (tests/batch_bsearch_streamed_cases.py;
tests/test_batch_bsearch_streamed_cpu.py asserts what each case covers), launch boundaries inside probes, a second call, the
degenerate options, no_defer_trick, an adaptor matrix that is not symmetric to the bit, J = 1, shared against per-problem
tables, the _feas loops, the host-driven form built from them, the oracle alone past n = 128, and the refusals."""
import numpy as np
import pytest

import batch_bsearch_reference as ref
import batch_bsearch_streamed_cases as cases
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SPACES = [False, True]
IDS = ["ell", "stable"]
N129 = cases.N129


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64 or b.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and np.array_equal(a, b)


def space_cls(gpu, stable):
    return gpu.EllStableBatchStreamed if stable else gpu.EllBatchStreamed


def make(gpu, n, B, stable, *, no_defer_trick=False):
    """(batch, problem) for the first B members of the family, on the streamed engines"""
    a, c, xc0 = ref.tables(n, B)
    batch = space_cls(gpu, stable).new_with_scalar(ref.KAPPA, xc0)
    prob = gpu.BatchLinFeasProblem.streamed(a, c)
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


def run_case(batch, prob, case, **kw):
    opts = dict(interval=case.interval, inner=case.inner, outer=case.outer)
    opts.update(kw)
    return prob.bsearch(batch, *opts["interval"], *opts["inner"], *opts["outer"])


def stacked(records):
    out = {k: np.array([w[k] for w in records]) for k in ("feasible", "niter", "upper", "rounds", "ends", "target", "xc")}
    out["niter"], out["rounds"] = out["niter"].astype(np.int64), out["rounds"].astype(np.int64)
    out["ends"] = out["ends"].astype(np.int64)
    out["idx"] = np.array([w["idx"] for w in records], dtype=np.int32)
    return out


# ---- the pin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_pin(gpu, stable):
    want = ref.pin(stable)
    assert want["feasible"] and want["niter"] == 34                                    # src/example3.rs:82-84
    batch = space_cls(gpu, stable).new_with_scalar(100.0, np.zeros((1, 2)))
    prob = gpu.BatchLinFeasProblem.streamed(np.array(ref.EX3_A), np.array(ref.EX3_C), 1)
    before = snapshot(batch)
    got = prob.bsearch(batch, -100.0, 100.0, 2000, 1e-8, 2000, 1e-8)
    one = {k: np.array([want[k]]) for k in ("feasible", "niter", "upper", "rounds", "idx", "target")}
    one["ends"], one["xc"] = np.array([want["ends"]]), want["xc"][None]
    check_run(batch, prob, got, one, before)


# ---- the family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES, ids=IDS)
@pytest.mark.parametrize("case", cases.FAMILY, ids=lambda c: c.id)
def test_family(gpu, case, stable):
    want = case.want(stable)
    batch, prob = make(gpu, case.n, case.B, stable)
    before = snapshot(batch)
    got = run_case(batch, prob, case)
    check_run(batch, prob, got, want, before)
    if case.n <= 128 and case.straddles:      # the last n of the LDS engines: their result on the same problems
        a, c, xc0 = ref.tables(case.n, case.B)
        lds = (gpu.EllStableBatch if stable else gpu.EllBatch).new_with_scalar(ref.KAPPA, xc0)
        plain = gpu.BatchLinFeasProblem(a, c)
        lds_before = snapshot(lds)
        lds_got = run_case(lds, plain, case)
        check_run(lds, plain, lds_got, want, lds_before)
        for u, v in zip(got, lds_got):
            assert same(u, v)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunks(gpu, chunk, stable):
    """chunk 1 puts a launch boundary inside every probe, on both sides of its first sweep"""
    for case in (N129, cases.FAMILY[1]):
        assert (case.n, case.B) in ((129, 4), (2, 9))
        want = case.want(stable)
        batch, prob = make(gpu, case.n, case.B, stable)
        prob.set_chunk(chunk)
        before = snapshot(batch)
        check_run(batch, prob, run_case(batch, prob, case), want, before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_second_call_continues(gpu, stable):
    B, half = 3, 0.5
    first, want = N129.want(stable, B=B), N129.want(stable, B=B, again=half)
    batch, prob = make(gpu, N129.n, B, stable)
    before = snapshot(batch)
    got = run_case(batch, prob, N129)
    check_run(batch, prob, got, first, before)
    check_run(batch, prob, prob.bsearch(batch, got[2] - half, got[2] + half, *N129.inner, *N129.outer), want, before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_degenerate_options(gpu, stable):
    n, B = 129, 3
    batch, prob = make(gpu, n, B, stable)
    before = snapshot(batch)
    (lo, up), inner = N129.interval, N129.inner
    idle = {"feasible": np.zeros(B, bool), "niter": np.zeros(B, np.int64), "upper": np.full(B, up),
            "rounds": np.zeros(B, np.int64), "ends": np.zeros((B, 4), np.int64), "idx": np.full(B, -1, np.int32),
            "target": np.full(B, -1e100), "xc": before[3]}
    check_run(batch, prob, prob.bsearch(batch, lo, up, *inner, 0, 1e-8), idle, before)           # max_iters = 0
    check_run(batch, prob, prob.bsearch(batch, lo, up, *inner, 2000, 201.0), idle, before)       # the first tau < tol
    check_run(batch, prob, prob.bsearch(batch, -3.0, -3.0, *inner, 2000, 1e-8),                  # lower == upper
              dict(idle, upper=np.full(B, -3.0)), before)
    # inner_max_iters = 0: every probe ends without an oracle call, the target moves
    want = ref.runs(n, B, stable, (0, 1e-8), (5, 1e-8), interval=N129.interval)
    assert not want["feasible"].any() and (want["ends"][:, 3] == 5).all() and (want["rounds"] == 0).all()
    assert (want["target"] != -1e100).all() and (want["idx"] == -1).all()
    check_run(batch, prob, prob.bsearch(batch, lo, up, 0, 1e-8, 5, 1e-8), want, before)


# ---- the host-driven form: what a user has with _feas_streamed alone ----------------------------------------------------------
def host_driven(batch, prob, lower, upper, inner, outer):
    """bsearch in numpy; each probe is a fresh streamed handle built from the getters, then set_target, feas, set_xc"""
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
    B = 3
    want = N129.want(stable, B=B)
    batch, prob = make(gpu, N129.n, B, stable)
    before = snapshot(batch)
    feasible, niter, upper, rounds = host_driven(batch, prob, *N129.interval, N129.inner, N129.outer)
    check_run(batch, prob, (feasible, niter, upper, rounds, want["ends"]), want, before)


# ---- variations ---------------------------------------------------------------------------------------------------------------
def test_no_defer_trick(gpu):
    B = 3
    want, plain = N129.want(False, B=B, no_defer_trick=True), N129.want(False, B=B)
    assert not same(want["xc"], plain["xc"])                   # the flag is seen: the clones' roundings differ
    batch, prob = make(gpu, N129.n, B, False, no_defer_trick=True)
    before = snapshot(batch)
    check_run(batch, prob, run_case(batch, prob, N129), want, before)


def unsymmetric(n, B):
    """[B][n][n], positive definite, the upper triangle one unit in the last place above the lower"""
    rng = np.random.default_rng(4242)
    out = []
    for _ in range(B):
        s = rng.standard_normal((n, n)) * 0.01
        m = np.eye(n) + s + s.T
        out.append(np.tril(m) + np.nextafter(np.tril(m, -1).T, np.inf))
    return np.stack(out)


def test_adaptor_matrix_that_is_not_symmetric(gpu):
    """the flag is clear: products walk true rows and a probe's first sweep mirrors the lower triangle into the probe
    buffer; the second call starts from the same unsymmetric matrix"""
    n, B, half = 129, 2, 0.5
    mq = unsymmetric(n, B)
    assert (mq != mq.transpose(0, 2, 1)).sum() == n * (n - 1) * B
    a, c, xc0 = ref.tables(n, B)
    batch = gpu.EllBatchStreamed.new_with_matrix(ref.KAPPA, mq, xc0)
    prob = gpu.BatchLinFeasProblem.streamed(a, c)
    before = snapshot(batch)
    assert same(before[0], mq)
    omegas = [ref.LinFeas(a[b], c[b]) for b in range(B)]
    spaces = [O.OracleEll.new_with_matrix(ref.KAPPA, mq[b], xc0[b]) for b in range(B)]
    first = [ref._record(om, sp, ref.bsearch(om, sp, *N129.interval, N129.inner, N129.outer)) for om, sp in zip(omegas, spaces)]
    want = stacked(first)
    assert want["ends"][:, 1:].sum() > 0 and (want["rounds"] >= 5 * want["niter"]).any()     # cuts, and probes that go on
    got = run_case(batch, prob, N129)
    check_run(batch, prob, got, want, before)
    again = [ref._record(om, sp, ref.bsearch(om, sp, w["upper"] - half, w["upper"] + half, N129.inner, N129.outer))
             for om, sp, w in zip(omegas, spaces, first)]
    assert all(same(np.array(sp.mq), mq[b]) for b, sp in enumerate(spaces))
    check_run(batch, prob, prob.bsearch(batch, got[2] - half, got[2] + half, *N129.inner, *N129.outer), stacked(again), before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_one_row(gpu, stable):
    """J = 1 at n = 129: the only row is the target's, and there are fewer rows than threads"""
    n, B = 129, 3
    interval, inner, outer = (-300.0, 0.0), (25, 1e-8), (12, 1e-8)
    rng = np.random.default_rng(5)
    a, xc0 = rng.standard_normal((B, 1, n)), rng.uniform(-0.2, 0.2, (B, n))
    batch = space_cls(gpu, stable).new_with_scalar(ref.KAPPA, xc0)
    prob = gpu.BatchLinFeasProblem.streamed(a, np.zeros((B, 1)))
    before = snapshot(batch)
    got = prob.bsearch(batch, *interval, *inner, *outer)
    want = []
    for b in range(B):
        omega, space = ref.LinFeas(a[b], [0.0]), ref.space_of(stable, xc0[b])
        want.append(ref._record(omega, space, ref.bsearch(omega, space, *interval, inner, outer)))
    want = stacked(want)
    assert want["feasible"].all() and (want["idx"] == 0).all()
    assert (want["ends"][:, 0] > 0).all() and (want["ends"][:, 1:].sum(axis=1) > 0).all()
    check_run(batch, prob, got, want, before)


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
def test_shared_table_equals_per_problem_tables(gpu, stable):
    n, B, member = 129, 4, 1
    a1, c1, x1 = ref.family(member, n)
    one = ref.run(member, n, stable, N129.inner, N129.outer, interval=N129.interval)
    results = []
    for per_problem in (False, True):
        batch = space_cls(gpu, stable).new_with_scalar(ref.KAPPA, np.tile(x1, (B, 1)))
        prob = gpu.BatchLinFeasProblem.streamed(np.tile(a1, (B, 1, 1)), np.tile(c1, (B, 1))) if per_problem else \
            gpu.BatchLinFeasProblem.streamed(a1, c1, B)
        results.append(run_case(batch, prob, N129) + prob.state() + (batch.xc(),))
    for u, v in zip(*results):
        assert same(u, v)
    assert same(results[0][2], np.full(B, one["upper"])) and same(results[0][3], np.full(B, one["rounds"], np.int64))
    assert same(results[0][7], np.tile(one["xc"], (B, 1)))


@pytest.mark.parametrize("n,B", [(129, 4), (1024, 2)])
def test_assess_feas(gpu, n, B):
    """past n = 128: one workgroup per problem"""
    a, c, xc0 = ref.tables(n, B)
    prob = gpu.BatchLinFeasProblem.streamed(a, c)
    omegas = [ref.LinFeas(a[b], c[b]) for b in range(B)]
    rng = np.random.default_rng(17)
    cuts = set()
    for call in range(6):
        if call == 3:
            gamma = rng.uniform(-3.0, 3.0, B)
            prob.set_target(gamma)
            for b in range(B):
                omegas[b].update(float(gamma[b]))
        x = rng.uniform(-4.0, 4.0, (B, n)) * (0.002 if call % 2 else 1.0)
        grad, beta, cut = prob.assess_feas(x)
        for b in range(B):
            w = omegas[b].assess_feas(x[b])
            if w is None:
                assert cut[b] == -1 and beta[b] == 0.0 and not grad[b].any()
            else:
                assert cut[b] == omegas[b].idx and same(grad[b], w[0]) and same(beta[b:b + 1], np.array([w[1]]))
            cuts.add(int(cut[b]))
        idx, target = prob.state()
        assert same(idx, np.array([o.idx for o in omegas], np.int32)) and same(target, np.array([o.target for o in omegas]))
    assert len(cuts) > 3 and max(cuts) >= n         # rows past the first n: a thread folds more than one row


FEAS_OFFSETS = {129: 25.0, 256: 70.0}   # above bsearch's optimum: some members find a point after 14 to 39 cuts, some none


@pytest.mark.parametrize("stable", SPACES, ids=IDS)
@pytest.mark.parametrize("n,B", [(129, 5), (256, 3)])
def test_feas(gpu, n, B, stable):
    a, c, xc0 = ref.tables(n, B)
    batch, prob = make(gpu, n, B, stable)
    case = N129 if n == 129 else cases.FAMILY[10]
    assert case.n == n
    optimum = ref.runs(n, B, False, case.inner, case.outer, interval=case.interval)["upper"]
    gamma = optimum + FEAS_OFFSETS[n]
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
        assert same(batch.kappa[b:b + 1], np.array([space.kappa])) and same(batch.tsq()[b:b + 1], np.array([space.tsq]))
    assert ref.END_FEASIBLE in ends and len(ends) > 1 and niter.max() >= 10
    idx, target = prob.state()
    assert same(target, gamma)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(gpu):
    n, B = 2, 9
    a, c, xc0 = ref.tables(n, B)
    prob = gpu.BatchLinFeasProblem.streamed(a, c)
    ell, stable = gpu.EllBatch.new_with_scalar(ref.KAPPA, xc0), gpu.EllStableBatch.new_with_scalar(ref.KAPPA, xc0)
    s_ell = gpu.EllBatchStreamed.new_with_scalar(ref.KAPPA, xc0)
    s_stable = gpu.EllStableBatchStreamed.new_with_scalar(ref.KAPPA, xc0)
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

    def call_feas(entry, batch, problem):
        out = [np.full((problem.B, problem.n), 7.0), np.full(problem.B, 7, np.int32), np.full(problem.B, 7, np.int64),
               np.full(problem.B, 7, np.int32)]
        before = snapshot(batch), problem.state()
        rc = getattr(lib, entry)(batch._h, problem._h, 25, 1e-8, *[o.ctypes.data for o in out])
        assert rc == E and lib.ellhip_last_error()
        assert all((o == 7).all() for o in out)
        after = snapshot(batch), problem.state()
        for u, v in zip(before[0] + before[1], after[0] + after[1]):
            assert same(u, v)

    se, ss = "ellhip_batch_linfeas_bsearch_streamed", "ellhip_batch_linfeas_bsearch_streamed_stable"
    fe, fs = "ellhip_batch_linfeas_feas_streamed", "ellhip_batch_linfeas_feas_streamed_stable"
    for entry in (se, ss):
        call(entry, ell, prob)                                  # LDS handles
        call(entry, stable, prob)
    for entry in (fe, fs):
        call_feas(entry, ell, prob)
        call_feas(entry, stable, prob)
    call(se, s_stable, prob)                                    # the wrong variant
    call(ss, s_ell, prob)
    call_feas(fe, s_stable, prob)
    call_feas(fs, s_ell, prob)
    text = call("ellhip_batch_linfeas_bsearch", s_ell, prob)    # the LDS entry points still refuse a streamed handle
    assert b"not built" in text and b"ellhip_batch_linfeas_bsearch_streamed" in text
    call("ellhip_batch_linfeas_bsearch_stable", s_stable, prob)
    other_b = gpu.BatchLinFeasProblem.streamed(*ref.tables(n, B + 1)[:2])
    call(se, s_ell, other_b)                                    # B
    call_feas(fe, s_ell, other_b)
    other_n = gpu.BatchLinFeasProblem.streamed(*ref.tables(3, B)[:2])
    call(se, s_ell, other_n)                                    # n
    call(ss, s_stable, other_n)
    call(se, s_ell, prob, lower=1.0, upper=0.5)                 # lower > upper
    call(ss, s_stable, prob, lower=1.0, upper=0.5)
    # an (n, J) whose block does not fit beside the LDS engines' matrices: refused by their check at call time
    wide = gpu.BatchLinFeasProblem.streamed(np.ones((4096, 128)), np.ones(4096), 2)
    lds128 = gpu.EllBatch.new_with_scalar(ref.KAPPA, np.zeros((2, 128)))
    assert b"more LDS" in call("ellhip_batch_linfeas_bsearch", lds128, wide)
    with pytest.raises(gpu.capi.EllHipError):
        wide.bsearch(lds128, -1.0, 1.0, 25, 1e-8, 10, 1e-8)
    plain = gpu.BatchLinFeasProblem(a, c)                       # the plain constructor keeps its dispatch
    with pytest.raises(gpu.capi.EllHipError):
        plain.feas(s_ell, 10, 1e-8)
    with pytest.raises(gpu.capi.EllHipError):
        plain.bsearch(s_ell, -50.0, 50.0, 25, 1e-8, 10, 1e-8)
    with pytest.raises(gpu.capi.EllHipError):
        prob.bsearch(s_stable, 1.0, 0.0, 25, 1e-8, 10, 1e-8)
    # and the handles still work, each on the engine of the batch handle it is given
    case = cases.FAMILY[1]
    for batch, st in ((s_ell, False), (s_stable, True), (ell, False), (stable, True)):
        before = snapshot(batch)
        problem = prob if batch is s_ell else gpu.BatchLinFeasProblem.streamed(a, c)   # prob: the one the refusals were given
        check_run(batch, problem, run_case(batch, problem, case), case.want(st), before)
