"""GPU: the batched device-resident max-cut loops on the LDS engines (include/ellhip_batch_maxcut.h:
ellhip_batch_maxcut_optim on Ell batch handles, ellhip_batch_maxcut_optim_stable on EllStable ones) against the reference's
MaxcutOracle restated in tests/batch_maxcut_reference.py and its cutting_plane_optim over the CPU oracle's spaces, and
against the host-driven form on the device.  The device keeps both of the oracle's folds in the reference's order, so every
comparison is EXACT (tests/batch_maxcut_checks.py): niter, status, gamma, has_best, x_best and the spaces afterwards (mq --
on EllStable the packed buffer with its scratch triangle -- xc, kappa, tsq)."""
import ctypes as C

import numpy as np
import pytest

import batch_maxcut_checks as chk
import batch_maxcut_reference as ref

pytestmark = pytest.mark.gpu

INF = np.inf
SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]
TABLES = [pytest.param(False, id="tables"), pytest.param(True, id="shared")]
# every T / epw shape: 64 instances of one thread; two threads; n = 3 does not divide 64; 16 in a workgroup; the odd pitch;
# the last n of 256 threads; the first of 128 and a single instance per workgroup; the largest
NS = [1, 2, 3, 16, 33, 64, 65, 128]


def max_iters_of(n):
    return 2000 if n <= 33 else 300   # some "mixed" members run past 2000 rounds from n = 64 on


@pytest.mark.parametrize("shared", TABLES)
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("n", NS)
def test_loop_against_the_cpu_runs(gpu, n, stable, shared):
    """B = 2 epw + 1: two full workgroups and a part-filled one, neighbours that stop at different rounds"""
    B = 2 * chk.lds_epw(n) + 1
    case = chk.family_batch(n, B, shared)
    max_iters = max_iters_of(n)
    recs = case.cpu_runs(stable, max_iters)
    if n >= 16:
        assert len({r["niter"] for r in recs}) > 1 and max(r["niter"] for r in recs) >= 20
        assert any(r["central"] >= 2 and r["deep"] >= 1 for r in recs)
    chk.check_loop(gpu, case, stable, False, recs, max_iters)


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("n", NS)
def test_loop_against_the_host_driven_form(gpu, n, stable):
    B = 2 * chk.lds_epw(n) + 1
    case = chk.family_batch(n, B)
    max_iters = min(max_iters_of(n), 120)
    prob = case.problem(gpu)
    batch = case.spaces(gpu, stable, False)
    got = prob.optim(batch, -INF, max_iters, ref.TOL)
    other = case.spaces(gpu, stable, False)
    recs = chk.host_driven(prob, other, max_iters)
    chk.assert_runs_equal(got, recs, n)
    chk.assert_state_equal(batch, recs)


@pytest.mark.parametrize("n,kind,max_iters,ell,stb", ref.ROWS, ids=ref.ROW_IDS)
def test_pinned_rows(gpu, n, kind, max_iters, ell, stb):
    """the pinned members s = 0..5 of tests/test_batch_maxcut_cpu.py, on both kinds of space"""
    sets = [ref.weights(s, n, kind) for s in range(6)]
    case = chk.Batch(np.stack([w for w, _ in sets]), np.stack([x for _, x in sets]))
    for stable, niters in ((False, ell), (True, stb)):
        recs = [ref.solve(s, n, kind, max_iters, ref.TOL, stable) for s in range(6)]
        _, _, got = chk.check_loop(gpu, case, stable, False, recs, max_iters)
        assert tuple(got[2].tolist()) == niters


def test_a_handle_of_another_kind_is_refused(gpu):
    lib = gpu.capi.load()
    n, B = 16, 5
    case = chk.family_batch(n, B)
    prob = case.problem(gpu)
    wide = chk.family_batch(129, 2).problem(gpu)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(entry, batch, oracle=prob):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        gamma = np.full(batch.B, 0.3)
        xb = np.full((batch.B, batch.n), np.nan)
        has = np.full(batch.B, -5, dtype=np.int32)
        niter = np.full(batch.B, -5, dtype=np.int64)
        status = np.full(batch.B, -5, dtype=np.int32)
        rc = getattr(lib, entry)(batch._h, oracle._h, ptr(gamma), 100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status))
        assert rc == gpu.capi.E_INVALID and lib.ellhip_last_error(), entry
        for a, b in zip(before, (batch.mq, batch.xc(), batch.kappa, batch.tsq())):
            assert chk.same_bits(a, b)
        assert np.isnan(xb).all() and (gamma == 0.3).all()
        assert (has == -5).all() and (niter == -5).all() and (status == -5).all()

    kinds = {"": (False, False), "_stable": (True, False), "_streamed": (False, True), "_streamed_stable": (True, True)}
    for suffix in kinds:
        for other, (stable, streamed) in kinds.items():
            if other != suffix:
                refused("ellhip_batch_maxcut_optim" + suffix, case.spaces(gpu, stable, streamed))
    rng = np.random.default_rng(2)
    refused("ellhip_batch_maxcut_optim", gpu.EllBatch.new_with_scalar(np.full(B + 1, 10.0), rng.standard_normal((B + 1, n))))
    refused("ellhip_batch_maxcut_optim", gpu.EllBatch.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n + 1))))
    # an oracle past the LDS engine's n has no LDS-engine handle to match
    refused("ellhip_batch_maxcut_optim", gpu.EllBatch.new_with_scalar(np.full(2, 10.0), rng.standard_normal((2, 128))), wide)
    refused("ellhip_batch_maxcut_optim_stable",
            gpu.EllStableBatch.new_with_scalar(np.full(2, 10.0), rng.standard_normal((2, 128))), wide)
    with pytest.raises(gpu.capi.EllHipError):
        prob.set_chunk(0)
    with pytest.raises(gpu.capi.EllHipError):
        prob.set_chunk(4097)
    with pytest.raises(gpu.capi.EllHipError):
        gpu.BatchMaxcutProblem(np.zeros((1025, 1025)), 2)
    with pytest.raises(ValueError):
        prob.assess_optim(np.zeros((B, n + 1)), -INF)
    # and the good pair still runs
    recs = case.cpu_runs(False, 2000)
    batch = case.spaces(gpu, False, False)
    chk.assert_runs_equal(prob.optim(batch, -INF, 2000, ref.TOL), recs, n)
    chk.assert_state_equal(batch, recs)
