"""GPU: the edges of the batched max-cut oracle and loops (include/ellhip_batch_maxcut.h): the reference's known answers,
tables that are not symmetric and carry a diagonal, centres holding -0.0 and NaN, the all-zero centre, ties between the cut
value and gamma, a NaN weight, chunking, max_iters = 0 and a second call.  Everything is compared as bit patterns against
tests/batch_maxcut_reference.py (tests/batch_maxcut_checks.py)."""
import numpy as np
import pytest

import batch_maxcut_checks as chk
import batch_maxcut_reference as ref

pytestmark = pytest.mark.gpu

INF = np.inf
SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]


def check_calls(prob, case, x, gamma):
    """one assess_optim of every problem at x [B][n] with gamma [B] against the restated oracle"""
    grad, beta, shrunk, gamma_out, cut = prob.assess_optim(x, gamma)
    gamma = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (case.B,))
    for b in range(case.B):
        (rg, rb), rs, rgamma, rcut = ref.assess_optim(case.table(b), x[b], gamma[b])
        chk.assert_bits(grad[b], rg, f"grad {b}")
        assert chk.same_bits(beta[b], rb) and chk.same_bits(gamma_out[b], rgamma) and chk.same_bits(cut[b], rcut), \
            (b, beta[b], gamma_out[b], cut[b], rb, rgamma, rcut)
        assert bool(shrunk[b]) == rs, b
    return grad, beta, shrunk, gamma_out, cut


def test_reference_known_answers(gpu):
    """src/oracles/maxcut_oracle.rs:57-83: w = [[0, 1], [1, 0]], x = [1, 1], gamma = -inf, twice"""
    w = np.array([[0.0, 1.0], [1.0, 0.0]])
    prob = gpu.BatchMaxcutProblem(w, 3)
    x = np.ones((3, 2))
    grad, beta, shrunk, gamma, cut = prob.assess_optim(x, -INF)
    assert shrunk.all()
    chk.assert_bits(gamma, np.zeros(3), "gamma")             # +0.0
    chk.assert_bits(cut, np.zeros(3), "cut_value")
    chk.assert_bits(beta, np.full(3, -0.0), "beta")          # -cut_value
    chk.assert_bits(grad, np.full((3, 2), -0.0), "grad")     # a zero sum is handed out as -0.0
    grad, beta, shrunk, gamma, cut = prob.assess_optim(x, gamma)
    assert not shrunk.any()
    chk.assert_bits(beta, np.zeros(3), "beta")               # gamma itself, +0.0
    chk.assert_bits(gamma, np.zeros(3), "gamma")
    chk.assert_bits(grad, np.full((3, 2), -0.0), "grad")
    # the optional outputs may be left out
    lib = gpu.capi.load()
    g, gm = np.zeros(3), np.empty((3, 2))
    p = lambda a: a.ctypes.data
    assert lib.ellhip_batch_maxcut_assess_optim(prob._h, p(x), p(g), p(gm), None, None, None) == 0
    chk.assert_bits(gm, np.full((3, 2), -0.0), "grad")


# the packed form at an odd n, at 16 instances a workgroup and at one; the wide form with a part-filled wave and at 1024
@pytest.mark.parametrize("n,B", [(1, 70), (5, 9), (16, 33), (128, 3), (130, 3), (1024, 2)])
def test_tables_that_are_not_symmetric_with_a_diagonal(gpu, n, B):
    """the gradient takes full rows, the value the upper triangle, nobody the diagonal; -0.0 and NaN in the centres"""
    rng = np.random.default_rng(100 + n)
    tables = rng.uniform(-1.0, 1.0, (B, n, n))
    tables[:, np.arange(n), np.arange(n)] = 1e6 * (1.0 + rng.random((B, n)))
    case = chk.Batch(tables, rng.normal(size=(B, n)))
    shared = chk.Batch(tables[B - 1], case.xc0, shared=True)
    for c in (case, shared):
        prob = c.problem(gpu)
        x = rng.normal(size=(B, n))
        _, _, shrunk, gamma, cut = check_calls(prob, c, x, -INF)
        assert shrunk.all() and (np.abs(cut) < 1e6).all()
        check_calls(prob, c, rng.normal(size=(B, n)), gamma)     # some improve on the first answer, some do not
        x = rng.choice(np.array([0.0, -0.0, np.nan, 1.0, -1.0, INF, -INF, 1e-310, -1e-310]), size=(B, n))
        x[0, 0], x[0, n - 1] = -0.0, np.nan
        grad, *_ = check_calls(prob, c, x, np.full(B, -INF))
        if n >= 5:
            assert not np.isnan(grad).any()
        # -0.0 counts as +1: the same answers as from +0.0
        x2 = np.where(x == 0.0, 0.0, x)
        chk.assert_bits(prob.assess_optim(x2, -INF)[0], grad, "grad")


def test_a_nan_weight_never_improves(gpu):
    n, B = 33, 4
    case = chk.family_batch(n, B)
    tables = case.tables.copy()
    tables[:, 3, 20] = np.nan   # the upper triangle only: the value and row 3 of the gradient
    case = chk.Batch(tables, case.xc0)
    x = case.xc0.copy()
    x[:, 3], x[:, 20] = 1.0, -1.0
    grad, beta, shrunk, gamma, cut = check_calls(case.problem(gpu), case, x, -INF)
    assert np.isnan(cut).all() and not shrunk.any() and (gamma == -INF).all() and (beta == -INF).all()
    assert np.isnan(grad[:, 3]).all() and np.isnan(grad).sum() == B


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("n,streamed", [(16, False), (130, True)])
def test_the_all_zero_centre(gpu, n, streamed, stable):
    """all signs equal: the gradient is all -0.0, omega = 0, and the reference's "Success" leaves a NaN state"""
    B = 3
    case = chk.family_batch(n, B)
    case = chk.Batch(case.tables, np.zeros((B, n)))
    recs = case.cpu_runs(stable, 5)
    for r in recs:
        assert np.isnan(r["xc"]).any() or np.isnan(r["tsq"]) or r["status"] != ref.SUCCESS
    chk.check_loop(gpu, case, stable, streamed, recs, 5)


@pytest.mark.parametrize("stable", SPACES)
def test_integer_weights_tie_with_gamma(gpu, stable):
    """small integer weights: cut values repeat, and a cut value equal to gamma is not an improvement"""
    n, B = 16, 9
    rng = np.random.default_rng(23)
    u = np.triu(rng.integers(-2, 3, (B, n, n)).astype(np.float64), 1)
    case = chk.Batch(u + np.swapaxes(u, 1, 2), rng.normal(size=(B, n)))
    recs = case.cpu_runs(stable, 2000)
    assert sum(r["ties"] for r in recs) >= 3 and max(r["niter"] for r in recs) >= 10
    chk.check_loop(gpu, case, stable, False, recs, 2000)


@pytest.mark.parametrize("chunk", [1, 7, 256])
@pytest.mark.parametrize("stable", SPACES)
def test_chunking_changes_nothing(gpu, stable, chunk):
    n, B = 16, 33
    case = chk.family_batch(n, B)
    recs = case.cpu_runs(stable, 2000)
    chk.check_loop(gpu, case, stable, False, recs, 2000, chunk=chunk)


@pytest.mark.parametrize("stable", SPACES)
def test_cut_off_resume_and_max_iters_zero(gpu, stable):
    n, B, first, more = 33, 15, 30, 2000
    case = chk.family_batch(n, B)
    spaces = case.cpu_spaces(stable)
    recs = case.cpu_runs(stable, first, spaces=spaces)
    assert {r["niter"] for r in recs} > {first}   # some stopped earlier, most were cut off
    prob, batch, got = chk.check_loop(gpu, case, stable, False, recs, first)
    # max_iters = 0 moves nothing: no x_best, gamma as given, the spaces as they were
    x_best, has, niter, gamma, status = prob.optim(batch, got[3], 0, ref.TOL)
    assert not has.any() and not niter.any() and not status.any() and np.isnan(x_best).all()
    chk.assert_bits(gamma, got[3], "gamma")
    chk.assert_state_equal(batch, recs)
    # the second call carries on: gamma carries over, x_best starts empty
    second = case.cpu_runs(stable, more, spaces=spaces, gamma=[r["gamma"] for r in recs])
    whole = case.cpu_runs(stable, first + more)
    for b in range(B):
        if recs[b]["niter"] == first:   # the uninterrupted run
            assert second[b]["niter"] + first == whole[b]["niter"]
            assert chk.same_bits(second[b]["xc"], whole[b]["xc"]) and chk.same_bits(second[b]["mq"], whole[b]["mq"])
            assert chk.same_bits(second[b]["gamma"], whole[b]["gamma"])
    got2 = prob.optim(batch, got[3], more, ref.TOL)
    chk.assert_runs_equal(got2, second, n)
    chk.assert_state_equal(batch, second)
