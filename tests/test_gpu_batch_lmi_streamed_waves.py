"""GPU: the batched LMI loops on streamed batch handles at 4, 5, 8 and 16 waves per workgroup, with the batches of
tests/batch_lmi_streamed_wave_cases.py: the factorisation stops late in a 64-block inside the loop (rows 59 ... 63: the long
witness solve and quadratic forms over nearly the whole block), in the middle and early; a second 64-block fails after a
first was factorised through every column; J = 8 blocks and the objective are walked and wrapped; NoSoln stands beside runs
that go on; n = 1023 and n = 257 leave one thread of the last wave idle or alone.  What the batches reach is asserted on the
CPU runs alone in tests/test_batch_lmi_streamed_waves_cpu.py, whose pins are checked here again.

Every comparison is that of tests/test_gpu_batch_lmi_streamed.py, whose helpers are used: float64 bit patterns and integers
against the cached CPU runs -- x_best / x, has_best / feasible, niter, status, gamma, idx and the spaces' matrix (EllStable:
the whole packed buffer), xc, kappa and tsq afterwards."""
import numpy as np
import pytest

import batch_lmi_streamed_cases as cases
import batch_lmi_streamed_wave_cases as waves
import test_batch_lmi_streamed_waves_cpu as pins
import test_gpu_batch_lmi_streamed as base
from test_gpu_batch_lmi_streamed import (INF, LOOPS, SPACES, assert_bits, assert_runs_equal, assert_state_equal, check_loop,
                                         cpu_runs, loop, new_spaces, same_bits)

pytestmark = pytest.mark.gpu


def shape_id(n, ms):
    return "%d-%s" % (n, "x".join(map(str, ms)))


# ---- 1. the pinned batches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", pins.PIN_KEYS, ids=pins.PIN_IDS)
def test_pinned_runs(gpu, key):
    bid, stable, feas = key
    n, ms, who, max_iters, tol, recs = waves.batch_records(bid, stable, feas)
    assert pins.summary(recs) == pins.PINS[key]
    check_loop(gpu, stable, feas, cases.stack(n, ms, who), recs, max_iters, tol)


# ---- 2. launches, stops and what lies between two calls ---------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("feas", LOOPS)
@pytest.mark.parametrize("chunk", [1, 7, 256])
@pytest.mark.parametrize("bid", ["1024-64", "257-8..1"])
def test_chunking_changes_nothing(gpu, bid, chunk, feas, stable):
    """chunk 1: the early oracle call is never made and no sweep is fused, so every late cut is followed by a plain sweep;
    7: six fused rounds, then a plain one; 256: one launch"""
    n, ms, who, max_iters, tol, recs = waves.batch_records(bid, stable, feas)
    check_loop(gpu, stable, feas, cases.stack(n, ms, who), recs, max_iters, tol, chunk=chunk)


# 1024-64: member t = 1.02 is cut off between its cuts at rows 59 and 61; 257-8..1 at 5: in mid-walk of the nine stations
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("feas", LOOPS)
@pytest.mark.parametrize("bid,first_iters", [("1024-64", 11), ("257-8..1", 5)])
def test_cut_off_and_resume(gpu, bid, first_iters, feas, stable):
    """cut off and resumed by a second call: idx and gamma carry over, and the whole equals one call"""
    n, ms, who, max_iters, tol, whole = waves.batch_records(bid, stable, feas)
    rest = max_iters - first_iters
    spaces_cpu = [cases.cpu_space(stable, *cases.start(s, n, ms, t)) for s, t in who]
    first = cpu_runs(stable, feas, n, ms, who, first_iters, 0.0, spaces=spaces_cpu)
    prob, spaces, got = check_loop(gpu, stable, feas, cases.stack(n, ms, who), first, first_iters, 0.0)
    gammas = None if feas else [r["gamma"] for r in first]
    second = cpu_runs(stable, feas, n, ms, who, rest, 0.0, spaces=spaces_cpu, gammas=gammas, idx=[r["idx"] for r in first])
    cut_off = 0
    for f, s, w in zip(first, second, whole):
        if f["niter"] == first_iters and not (feas and f["x"] is not None):   # cut off, not ended: the two calls make the one run
            assert f["niter"] + s["niter"] == w["niter"] and same_bits(s["mq"], w["mq"]) and s["idx"] == w["idx"]
            cut_off += 1
    assert cut_off >= 2
    if bid == "257-8..1":   # the index stood at several stations when the first call ended, the objective among them
        assert len({r["idx"] for r in first}) >= 3 and (feas or len(ms) in {r["idx"] for r in first})
    got2 = loop(prob, spaces, feas, rest, 0.0, INF if feas else got[4])
    assert_runs_equal(got2, second, n)
    assert_state_equal(prob, spaces, second)


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("feas", LOOPS)
@pytest.mark.parametrize("bid", ["1024-64", "512-64x64"])
def test_shared_pencil_equals_the_pencil_given_b_times(gpu, bid, feas, stable):
    """one pencil, B different B_j, c and starts: shared_f = 1 against the same pencil stacked B times, and the CPU"""
    n, ms, who, max_iters, tol = waves.BATCHES[bid]
    mat_f, mat_b, c, kappa, xc = cases.stack(n, ms, who)
    recs = cpu_runs(stable, feas, n, ms, who, max_iters, tol, shared=True)
    assert len({r["niter"] for r in recs}) > 1 or not feas
    assert any(st < len(ms) for r in recs for st in r["stations"][1:])   # block cuts inside the loop
    a = check_loop(gpu, stable, feas, (mat_f, mat_b, c, kappa, xc), recs, max_iters, tol, shared=True)
    tiled = [np.broadcast_to(f[0], f.shape).copy() for f in mat_f]
    b = check_loop(gpu, stable, feas, (tiled, mat_b, c, kappa, xc), recs, max_iters, tol)
    assert a[0].shared and not b[0].shared
    for g, w in zip(a[2], b[2]):
        assert (g is None and w is None) or same_bits(g.astype(np.float64), w.astype(np.float64))
    assert_bits(a[1].mq, b[1].mq, "mq")


@pytest.mark.parametrize("stable", SPACES)
def test_populated_start(gpu, stable):
    """1024-64 from spaces that took five batch updates first: on Ell the first sweep inside the loop reads a dense matrix.
    From there member t = 1.02 is cut at rows 55 ... 63 of the 64-block, with objective cuts in between"""
    n, ms, who, max_iters, tol = waves.BATCHES["1024-64"]
    B, K = len(who), 5
    stacked = cases.stack(n, ms, who)
    spaces = new_spaces(gpu, stable, stacked[3], stacked[4])
    spaces_cpu = [cases.cpu_space(stable, *cases.start(s, n, ms, t)) for s, t in who]
    rng = np.random.default_rng(1024)
    grads = rng.standard_normal((K, B, n))
    kinds = rng.integers(0, 2, size=(K, B)).astype(np.int32)
    beta = np.zeros((K, B))
    want = np.zeros((K, B), dtype=np.int32)
    for k in range(K):
        for b, space in enumerate(spaces_cpu):
            beta[k, b] = 0.1 * np.sqrt(space.tsq) if kinds[k, b] == 0 else 0.0
            want[k, b] = space.update(int(kinds[k, b]), grads[k, b], beta[k, b])
    assert (beta[1:] > 0.0).any() and not want.any()
    status, _ = spaces.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    mq = np.stack([np.array(space.mq) for space in spaces_cpu])
    assert_bits(spaces.mq, mq, "mq before the loop")
    assert stable or np.count_nonzero(mq) == mq.size   # (the CPU oracle's EllStable matrix is still diagonal here)
    recs = cpu_runs(stable, False, n, ms, who, max_iters, tol, spaces=spaces_cpu)
    assert max(row for r in recs for row in r["rows"][1:]) >= 62
    check_loop(gpu, stable, False, stacked, recs, max_iters, tol, spaces=spaces)


# ---- 3. the oracle call by call at 4 to 10 waves ----------------------------------------------------------------------------
# two 64-blocks; J = 8 with one live thread in the last wave; four waves; ten waves with m(m+1)/2 = 561, 2080 and 1 elements,
# below n, above 3 n and one.  In the LMI0 form the triangle copy's `s = 0.0; s += ...` branch runs at these widths.
CALL_SHAPES = [(512, (64, 64)), (257, (8, 7, 6, 5, 4, 3, 2, 1)), (193, (64, 5)), (640, (33, 64, 1))]


@pytest.mark.parametrize("n,ms", CALL_SHAPES, ids=[shape_id(n, ms) for n, ms in CALL_SHAPES])
def test_oracle_call_by_call(gpu, n, ms):
    assert len(base.FORMS) == 4 and any(lmi0 for lmi0, _, _ in base.FORMS)
    base.oracle_call_by_call(gpu, n, ms)
