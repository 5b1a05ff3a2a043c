"""GPU: the batched device-resident max-cut loops on the streamed engines (include/ellhip_batch_maxcut.h:
ellhip_batch_maxcut_optim_streamed on streamed Ell batch handles, ellhip_batch_maxcut_optim_streamed_stable on streamed
EllStable ones): at n the LDS engines take too against the LDS engines' results, past it against the reference's
MaxcutOracle restated in tests/batch_maxcut_reference.py and its cutting_plane_optim over the CPU oracle's spaces.  Every
comparison is EXACT (tests/batch_maxcut_checks.py): niter, status, gamma, has_best, x_best and the spaces afterwards (mq -- on
EllStable the packed buffer with its scratch triangle -- xc, kappa, tsq)."""
import numpy as np
import pytest

import batch_maxcut_checks as chk
import batch_maxcut_reference as ref

pytestmark = pytest.mark.gpu

INF = np.inf
SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]
TABLES = [pytest.param(False, id="tables"), pytest.param(True, id="shared")]


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("n,B,max_iters", [(16, 7, 2000), (128, 3, 150)])
def test_streamed_equals_the_lds_engine(gpu, n, B, max_iters, stable):
    """one wave with 48 idle lanes, and two full waves: the same problems on both engines, from one oracle handle"""
    case = chk.family_batch(n, B)
    prob = case.problem(gpu)
    lds = case.spaces(gpu, stable, False)
    recs = chk.device_records(prob.optim(lds, -INF, max_iters, ref.TOL), lds)
    assert len({r["niter"] for r in recs}) > 1 and max(r["niter"] for r in recs) >= 20
    streamed = case.spaces(gpu, stable, True)
    chk.assert_runs_equal(prob.optim(streamed, -INF, max_iters, ref.TOL), recs, n)
    chk.assert_state_equal(streamed, recs)


# a part-filled last wave (129 threads of 192), 4 waves, 16 waves; at n = 1024 a few rounds, enough that a deep cut follows
# the first central one
@pytest.mark.parametrize("shared", TABLES)
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("n,max_iters", [(129, 60), (256, 40), (1024, 4)])
def test_loop_against_the_cpu_runs(gpu, n, max_iters, stable, shared):
    case = chk.family_batch(n, 3, shared)
    recs = case.cpu_runs(stable, max_iters)
    assert any(r["central"] >= 1 and r["deep"] >= 1 for r in recs)
    if not shared:
        assert len({r["niter"] for r in recs}) > 1   # the "pos" member stops early, the others are cut off
    chk.check_loop(gpu, case, stable, True, recs, max_iters)


@pytest.mark.parametrize("stable", SPACES)
def test_tables_that_are_not_symmetric(gpu, stable):
    """two copies on the device: the value reads the row-major one, the gradient the transposed one (n = 129: the transpose
    has part-filled tiles in both directions, three tables)"""
    n, B, max_iters = 129, 3, 30
    rng = np.random.default_rng(17)
    case = chk.Batch(rng.uniform(-1.0, 1.0, (B, n, n)), rng.normal(size=(B, n)))
    recs = case.cpu_runs(stable, max_iters)
    assert any(r["central"] >= 1 and r["deep"] >= 1 for r in recs)
    chk.check_loop(gpu, case, stable, True, recs, max_iters)


@pytest.mark.parametrize("stable", SPACES)
def test_chunks_and_a_second_call(gpu, stable):
    """n = 129: launches of one and of seven rounds against one launch, then a second call that carries on"""
    n, B, first, more = 129, 3, 20, 25
    case = chk.family_batch(n, B)
    spaces = case.cpu_spaces(stable)
    recs = case.cpu_runs(stable, first, spaces=spaces)
    for chunk in (1, 7):
        chk.check_loop(gpu, case, stable, True, recs, first, chunk=chunk)
    prob, batch, got = chk.check_loop(gpu, case, stable, True, recs, first)
    live = [b for b in range(B) if recs[b]["niter"] == first]
    assert live and len(live) < B
    second = case.cpu_runs(stable, more, spaces=spaces, gamma=[r["gamma"] for r in recs])
    whole = case.cpu_runs(stable, first + more)
    for b in live:   # the uninterrupted run
        assert second[b]["niter"] + first == whole[b]["niter"] and chk.same_bits(second[b]["xc"], whole[b]["xc"])
    got2 = prob.optim(batch, got[3], more, ref.TOL)
    chk.assert_runs_equal(got2, second, n)
    chk.assert_state_equal(batch, second)
