"""GPU: the streamed low-pass loops (k_batch_streamed_loop on an EllBatchStreamed; k_batch_streamed_loop_stable on
an EllStableBatchStreamed) past the first passband rows, at blocks of 4, 8 and 16 waves.  The other tests of
these kernels start from new_with_scalar(40, 0), where every oracle call stops at one of the first passband rows; here the
six members of tests/lowpass_warm_starts.py start from new_with_scalar(1e-3, x0) and within 30 rounds walk the whole table,
take every return of assess_feas / assess_optim, find feasible points, write x_best, lower gamma, issue the CENTRAL update
of a shrunk cut and end their `_feas` runs at round 0, late and never in one launch
(tests/test_lowpass_warm_starts_cpu.py checks and pins all of that on the CPU loop alone).

Every comparison is the one of tests/test_gpu_batch_lowpass_streamed_stable.py (assert_records_equal): float64 bit patterns,
NaN by position, and integers -- niter, status, has_best, gamma, x_best, the oracle state (cursors, kmax, fmax, more_alt,
sp_sq), Q or the packed buffer with its scratch triangle, xc, kappa and tsq.  No tolerances."""
import collections
import functools

import numpy as np
import pytest

import batch_lowpass_reference as lp
import batch_stable_loop_reference as ref
import lowpass_warm_starts as ws
import test_gpu_batch_lowpass_streamed_stable as stb
from util import dense_spd

pytestmark = pytest.mark.gpu

ROUNDS = 30
both = pytest.mark.parametrize("stable", [False, True], ids=["Ell", "EllStable"])
kinds = pytest.mark.parametrize("feas", [False, True], ids=["optim", "feas"])


# ---- one way to run either engine ---------------------------------------------------------------------------------------------
def make_batch(gpu, stable, case, lds=False):
    if stable:
        return stb.make_batch(gpu, case, gpu.EllStableBatch if lds else None)
    cls = gpu.EllBatch if lds else gpu.EllBatchStreamed
    if case.mq is None:
        batch = cls.new_with_scalar(case.kappa, case.xc)
    else:
        batch = cls.new_with_matrix(case.kappa, case.mq, case.xc)
    assert batch.variant == gpu.capi.SPACE_ELL and (batch.B, batch.n) == (case.B, case.n)
    if not case.use_parallel:
        batch.set_use_parallel_cut(False)
    return batch


def make_prob(gpu, case, chunk=None, lds=False):
    make = gpu.BatchLowpassProblem if lds else gpu.BatchLowpassProblem.streamed
    prob = make(case.n, *lp.columns(case.problems))
    if chunk is not None:
        prob.set_chunk(chunk)
    return prob


def run(gpu, stable, case, *, prob=None, batch=None, chunk=None, lds=False, **kw):
    """-> the records of stb.run_device (which asserts that rows of x_best without a result stay NaN)"""
    prob = make_prob(gpu, case, chunk, lds) if prob is None else prob
    batch = make_batch(gpu, stable, case, lds) if batch is None else batch
    assert lds or batch.is_streamed
    return stb.run_device(prob, batch, case, **kw)


def check(gpu, stable, case, want, what, **kw):
    got = run(gpu, stable, case, **kw)
    stb.assert_records_equal(got, want, f"{'EllStable' if stable else 'Ell'} {what} ({case.kind}, n = {case.n})")
    return got


def assert_results(want, consts, feas):
    """on the CPU records: the runs do what the tests are for"""
    if feas:   # three different ends in one launch: at once, late, at the cap
        assert want[0]["niter"] == 0 and want[0]["x_best"] is not None
        assert 0 < want[2]["niter"] < ROUNDS and want[2]["x_best"] is not None and want[2]["status"] == ref.SUCCESS
        assert want[1]["niter"] == ROUNDS and want[1]["x_best"] is None
    else:      # autocorr and transition shrink
        for m in (0, 2):
            assert want[m]["x_best"] is not None and want[m]["gamma"] < consts[m][4] and want[m]["niter"] == ROUNDS


# ---- 1. the deep walk and its results -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [193, 512, 1023])
@kinds
@both
def test_deep_walk_and_results(gpu, stable, feas, n):
    """4 waves with one thread in the last, 8 full waves, 16 waves with a padded last one"""
    case = ws.warm_case(n, feas=feas, rounds=ROUNDS)
    want = ws.warm_records(n, stable, feas, ROUNDS)
    assert_results(want, case.problems, feas)
    check(gpu, stable, case, want, "warm batch")


@functools.lru_cache(maxsize=None)
def starts1024():
    """The six members and a seventh, 0.9 * lowpass_autocorr: at this n Ell's transition member shrinks only once within 40
    rounds, and two members are to shrink twice and go on."""
    return ws.starts(1024) + [(ws.LOOSE, 0.9 * ws.lowpass_autocorr(1024))]


@pytest.fixture(scope="module")
def prob1024(gpu):
    """the n = 1024 table is 240 MiB: one handle of the members' constants for the module, for both engines (the handles of
    the two older files hold two problems of other constants)"""
    prob = gpu.BatchLowpassProblem.streamed(1024, *lp.columns([c for c, _ in starts1024()]))
    yield prob
    del prob


@functools.lru_cache(maxsize=None)
def traces1024(stable, feas):
    return [ws.trace(1024, c, x0, stable, ROUNDS, feas=feas) for c, x0 in starts1024()]


@kinds
@both
def test_n1024(gpu, prob1024, stable, feas):
    """16 full waves.  The CPU records are the hand-stepped loop's (ws.trace), so that the conditions of
    tests/test_lowpass_warm_starts_cpu.py, which leaves this size out, are checked here on the records compared with."""
    consts = [c for c, _ in starts1024()]
    case = ws.warm_case(1024, feas=feas, rounds=ROUNDS, pairs=starts1024())
    want = traces1024(stable, feas)
    assert_results(want, consts, feas)
    reached = collections.Counter(s for t in want for s in t["sites"])
    if feas:
        assert reached[ws.FEASIBLE] == 4 and ws.FEASIBLE not in want[1]["sites"]
        assert all(reached[s] >= 1 for s in (ws.PASS_HIGH, ws.PASS_LOW, ws.STOP_NEGATIVE, ws.TRANSITION_NEGATIVE, ws.X0_NEGATIVE))
    else:
        assert all(reached[s] >= 1 for s in ws.SITES if s != ws.FEASIBLE), reached
        twice = [t for t in want if sum(s == ws.SHRUNK for s in t["sites"][:-1]) >= 2]   # each followed by a further cut
        assert len(twice) >= 2
    assert np.mean([r for t in want for r in t["rows"]]) > 2.0
    stb.as_new(prob1024, consts)
    check(gpu, stable, case, want, "warm batch", prob=prob1024)


# ---- 2. populated factors -----------------------------------------------------------------------------------------------------
def populated_case(n, stable):
    case = ws.warm_case(n, rounds=ROUNDS)
    if stable:
        return case.with_random_factors(n)
    case.mq = np.stack([dense_spd(n, 100 * n + m) for m in range(case.B)])
    return case


@pytest.mark.parametrize("n", [512, 1023])
@both
def test_populated_factors(gpu, stable, n):
    """A shrunk round meets a full factor and scratch triangle (EllStable: with_random_factors(n), with the kappa in
    [0.0005, 1.0005) that it draws, unscaled) or a dense Q (Ell: util.dense_spd as it is, kappa = 1e-3: the autocorrelation
    member is still feasible at round 0).  Within the 30 rounds the autocorrelation and the transition member both shrink on
    the CPU, in both spaces and at both sizes."""
    case = populated_case(n, stable)
    want, _ = ws.cpu_run(case, stable)
    for m in (0, 2):
        assert want[m]["x_best"] is not None and want[m]["gamma"] < case.problems[m][4]
    assert max(w["niter"] for w in want) == ROUNDS
    tri = np.tril if stable else np.triu
    assert all(np.count_nonzero(tri(w["mq"], -1 if stable else 1)) > n * (n - 1) // 2 * 9 // 10 for w in want)
    check(gpu, stable, case, want, "populated factors")


# ---- 3. launch boundaries on a shrunk round -----------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 256])
@both
def test_chunking_changes_nothing(gpu, stable, chunk):
    """chunk 1: every round is a launch of its own, so every shrunk round's carried state crosses one"""
    check(gpu, stable, ws.warm_case(512, rounds=ROUNDS), ws.warm_records(512, stable, False, ROUNDS), f"chunk {chunk}", chunk=chunk)


@pytest.mark.parametrize("member", [3, 2], ids=["negative-x0", "transition"])
@both
def test_cut_off_before_the_first_shrunk_round_and_continue(gpu, stable, member):
    n = 512
    c, x0 = ws.starts(n)[member]
    sites = ws.trace(n, c, x0, stable, ROUNDS)["sites"]
    k = sites.index(ws.SHRUNK)   # the member's first shrunk round is the first round of the second call
    assert 1 <= k < ROUNDS - 1
    case = ws.warm_case(n, rounds=ROUNDS)
    full = ws.warm_records(n, stable, False, ROUNDS)
    first, live = ws.cpu_run(case, stable, max_iters=k)
    second, _ = ws.cpu_run(case, stable, max_iters=ROUNDS - k, resume=live)
    assert first[member]["niter"] == k and second[member]["niter"] == ROUNDS - k and second[member]["x_best"] is not None
    running = [m for m, a in enumerate(first) if a["niter"] == k and a["status"] == ref.SUCCESS]
    assert len(running) >= 5   # (Ell's negative-x0 member under LOOSE ends NoSoln at round 13; a second call asks its oracle again)
    for a, b, f in ((first[m], second[m], full[m]) for m in running):   # the CPU run driven this way is the uninterrupted run
        assert a["niter"] + b["niter"] == f["niter"] and b["status"] == f["status"] and b["state"] == f["state"]
        assert b["gamma"] == f["gamma"] and b["tsq"] == f["tsq"] and b["kappa"] == f["kappa"]
        assert np.array_equal(b["mq"], f["mq"]) and np.array_equal(b["xc"], f["xc"])
    prob, batch = make_prob(gpu, case), make_batch(gpu, stable, case)
    got = check(gpu, stable, case, first, f"cut off at {k}", prob=prob, batch=batch, max_iters=k)
    check(gpu, stable, case, second, "continued", prob=prob, batch=batch, max_iters=ROUNDS - k,
          gamma=np.array([g["gamma"] for g in got]))


# ---- 4. the host-driven form ----------------------------------------------------------------------------------------------------
@kinds
def test_equals_the_host_driven_form(gpu, feas):
    """EllStable, n = 512: the CPU oracle per instance and ellhip_batch_update with K = 1, with the NoSoln cut parked on the
    members that have stopped (a feasible point at round 0, 1 and 17; optim: none stops)"""
    case = ws.warm_case(512, feas=feas, rounds=ROUNDS)
    want = ws.warm_records(512, True, feas, ROUNDS)
    hosted = ref.host_driven(stb.make_batch(gpu, case), case)
    stb.assert_records_equal(hosted, want, "host-driven vs CPU")
    stb.assert_records_equal(run(gpu, True, case), hosted, "device loop vs host-driven")


# ---- 5. use_parallel_cut off ------------------------------------------------------------------------------------------------------
@kinds
@both
def test_without_parallel_cuts(gpu, stable, feas):
    """the parallel cuts of these starts fall back to deep cuts"""
    plain = ws.warm_records(512, stable, feas, ROUNDS)
    want = ws.warm_records(512, stable, feas, ROUNDS, None, False)
    for m in (1, 5):   # 30 parallel cuts each, in the passband and past it: the flag does something
        assert not np.array_equal(plain[m]["xc"], want[m]["xc"])
    if not feas:
        assert want[0]["x_best"] is not None and want[0]["gamma"] < ws.LOOSE[4]
    check(gpu, stable, ws.warm_case(512, feas=feas, rounds=ROUNDS, use_parallel=False), want, "use_parallel_cut off")


# ---- 6. across engines ------------------------------------------------------------------------------------------------------------
@kinds
@both
def test_equals_the_lds_engine(gpu, stable, feas):
    """n = 128: the LDS engine's loops (ellhip_batch_lowpass_{optim,feas} and their _stable forms) and the streamed kernels,
    which run a two-wave block there"""
    case = ws.warm_case(128, feas=feas, rounds=ROUNDS)
    want = ws.warm_records(128, stable, feas, ROUNDS)
    assert_results(want, case.problems, feas)
    got_l = check(gpu, stable, case, want, "LDS engine", lds=True)
    got_s = check(gpu, stable, case, want, "streamed engine")
    stb.assert_records_equal(got_s, got_l, "streamed vs LDS engine")
