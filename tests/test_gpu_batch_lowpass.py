"""GPU: the batched device-resident low-pass design loop (include/ellhip_batch_lowpass.h) against the CPU oracle
(oracle.OracleLowpass over OracleEll, through tests/batch_lowpass_reference.py).  The device oracle folds every row . x
left to right like the CPU and writes every beta as the reference does, so every comparison is EXACT: == on float64 bits
and on integers -- gradient, beta0, has_beta1, beta1, shrunk, gamma, the oracle state (cursors, kmax, fmax, more_alt,
sp_sq), x_best, has_best, niter, status and the spaces' Q, xc, kappa and tsq afterwards."""
import ctypes as C

import numpy as np
import pytest

import batch_lowpass_reference as ref
from lowpass_probes import CONSTANT_SETS, negative_x0_probe, probe_points, transition_probe

pytestmark = pytest.mark.gpu

MAX_ITERS, TOL = ref.MAX_ITERS, ref.TOL


def make_gpu(gpu, n, consts_list, chunk=None):
    B = len(consts_list)
    prob = gpu.BatchLowpassProblem(n, *ref.columns(consts_list))
    batch = gpu.EllBatch.new_with_scalar(np.full(B, ref.KAPPA), np.zeros((B, n)))
    if chunk is not None:
        prob.set_chunk(chunk)
    return prob, batch


def assert_state_equal(prob, states, what=""):
    got, want = prob.state(), ref.stack_state(states)
    for k in ref.STATE_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")


def assert_spaces_equal(batch, recs):
    np.testing.assert_array_equal(batch.mq, np.stack([np.array(r["mq"]) for r in recs]))
    np.testing.assert_array_equal(batch.xc(), np.stack([np.array(r["xc"]) for r in recs]))
    np.testing.assert_array_equal(batch.kappa, np.array([r["kappa"] for r in recs]))
    np.testing.assert_array_equal(batch.tsq(), np.array([r["tsq"] for r in recs]))


def assert_runs_equal(got, recs, n):
    x_best, has, niter, gamma, status = got
    np.testing.assert_array_equal(niter, np.array([r["niter"] for r in recs], dtype=np.int64))
    np.testing.assert_array_equal(status, np.array([r["status"] for r in recs], dtype=np.int32))
    np.testing.assert_array_equal(has, np.array([r["x_best"] is not None for r in recs], dtype=np.int32))
    if gamma is not None:
        np.testing.assert_array_equal(gamma, np.array([r["gamma"] for r in recs]))
    want = np.stack([np.full(n, np.nan) if r["x_best"] is None else r["x_best"] for r in recs])
    np.testing.assert_array_equal(x_best, want)  # rows without a result stay as the caller left them (NaN)


def check_optim(gpu, n, consts_list, max_iters=MAX_ITERS, tol=TOL, chunk=None):
    recs = [ref.solve_optim(n, tuple(c), max_iters, tol) for c in consts_list]
    prob, batch = make_gpu(gpu, n, consts_list, chunk)
    got = prob.optim(batch, np.array([c[4] for c in consts_list]), max_iters, tol)
    assert_runs_equal(got, recs, n)
    assert_state_equal(prob, [r["state"] for r in recs])
    assert_spaces_equal(batch, recs)
    return recs


def check_feas(gpu, n, consts_list, max_iters=MAX_ITERS, tol=TOL):
    recs = [ref.solve_feas(n, tuple(c), max_iters, tol) for c in consts_list]
    prob, batch = make_gpu(gpu, n, consts_list)
    x, ok, niter, status = prob.feas(batch, max_iters, tol)
    assert_runs_equal((x, ok, niter, None, status), recs, n)
    assert_state_equal(prob, [r["state"] for r in recs])
    assert_spaces_equal(batch, recs)
    return recs


# ---- 1. the oracle call by call ---------------------------------------------------------------------------------------
def where_it_returned(omega, cut):
    """which return statement of assess_feas (src/oracles/lowpass_oracle.rs:58-133) the CPU call just took"""
    if cut is None:
        return "none"
    s = omega.state()
    if not s["more_alt"]:
        return "x0"
    visited, sign = omega.s.rows_visited, "pos" if cut[0][0] == 1.0 else "neg"  # row[0] is 1.0
    if visited <= s["nwpass"]:
        return "pass_" + sign
    if visited <= s["nwpass"] + (15 * omega.n - s["nwstop"]):
        return "stop_" + sign
    return "transition"


def compare_feas_calls(prob, omegas, xs, seen):
    B, n = len(omegas), omegas[0].n
    for it, x in enumerate(xs):
        want = [o.assess_feas(x) for o in omegas]
        for o, w in zip(omegas, want):
            seen.add(where_it_returned(o, w))
        grad, b0, has1, b1, cut = prob.assess_feas(np.tile(x, (B, 1)))
        for b, w in enumerate(want):
            assert cut[b] == (w is not None), (it, b)
            if w is None:
                assert np.isnan(grad[b]).all() and np.isnan(b0[b])  # untouched
                continue
            g, (w0, w1) = w
            np.testing.assert_array_equal(grad[b], g, err_msg=f"call {it} instance {b}")
            assert b0[b] == w0 and has1[b] == (w1 is not None) and (w1 is None or b1[b] == w1), (it, b, b0[b], b1[b], w)
        assert_state_equal(prob, [o.state() for o in omegas], f"call {it}")


@pytest.mark.parametrize("n", [4, 9, 16, 33, 64, 128])
def test_oracle_call_by_call(gpu, orc, n):
    names = sorted(CONSTANT_SETS)
    consts = [tuple(CONSTANT_SETS[k]) for k in names]
    omegas = [orc.OracleLowpass(n, *c) for c in consts]
    prob = gpu.BatchLowpassProblem(n, *ref.columns(consts))
    np.testing.assert_array_equal(prob.spectrum, omegas[0].spectrum)
    assert_state_equal(prob, [o.state() for o in omegas], "new")
    xs = list(probe_points(n, np.random.default_rng(7 + n), 40))
    if n == 128:
        e0 = np.eye(n)[0]
        xs += [transition_probe(n), negative_x0_probe(n), 0.5 * e0, 2.0 * e0, 0.1 * e0, e0]
    seen = set()
    compare_feas_calls(prob, omegas, xs, seen)
    if n == 128:  # asserted on the CPU side: the calls reach every return statement
        assert seen == {"pass_pos", "pass_neg", "stop_pos", "stop_neg", "transition", "x0", "none"}, seen

    # assess_optim on two of the sets
    consts = [tuple(CONSTANT_SETS["corrected"]), tuple(CONSTANT_SETS["very_loose"])]
    omegas = [orc.OracleLowpass(n, *c) for c in consts]
    prob = gpu.BatchLowpassProblem(n, *ref.columns(consts))
    gamma = np.array([c[4] for c in consts])
    nshrunk = 0
    for it, x in enumerate(probe_points(n, np.random.default_rng(n), 12)):
        grad, b0, has1, b1, shrunk, gamma_out, rc = prob.assess_optim(np.tile(x, (2, 1)), gamma)
        for b, o in enumerate(omegas):
            (g, (w0, w1)), sh, ga = o.assess_optim(x, gamma[b])
            assert rc[b] == 1 and shrunk[b] == sh and gamma_out[b] == ga, (it, b)
            np.testing.assert_array_equal(grad[b], g)
            assert b0[b] == w0 and has1[b] == (w1 is not None) and (w1 is None or b1[b] == w1), (it, b)
            nshrunk += sh
        assert_state_equal(prob, [o.state() for o in omegas], f"optim call {it}")
        gamma = gamma_out
    if n >= 64:
        assert nshrunk > 0


def test_assess_optim_without_a_stopband_answers_state_error(gpu, orc):
    n = 8
    consts = [ref.NO_STOPBAND_A, ref.LOOSE]
    prob = gpu.BatchLowpassProblem(n, *ref.columns(consts))
    x = np.eye(n)[0]  # flat spectrum 1.0: inside the passband limits of both
    omegas = [orc.OracleLowpass(n, *c) for c in consts]
    with pytest.raises(IndexError):
        omegas[0].assess_optim(x, 0.3)
    (g, (w0, w1)), sh, ga = omegas[1].assess_optim(x, 0.3)
    grad, b0, has1, b1, shrunk, gamma, rc = prob.assess_optim(np.tile(x, (2, 1)), 0.3)
    assert rc[0] == gpu.capi.E_STATE and np.isnan(grad[0]).all() and gamma[0] == 0.3 and shrunk[0] == 0
    assert rc[1] == 1 and shrunk[1] == sh and gamma[1] == ga and b0[1] == w0 and b1[1] == w1
    np.testing.assert_array_equal(grad[1], g)
    assert_state_equal(prob, [o.state() for o in omegas])


# ---- 2. pinned runs as copies -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 257])
def test_short_passband_copies(gpu, B):
    recs = check_optim(gpu, 32, [ref.SHORT_PASSBAND] * B)
    assert recs[0]["niter"] == 969 and recs[0]["gamma"] == 2.1710931196961606e-08


# ---- 3. the table of pins ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,consts,B,niter,status", [
    (32, ref.CORRECTED, 3, 12481, ref.SUCCESS), (48, ref.CORRECTED, 1, 6693, ref.SUCCESS),
    (32, ref.AS_WRITTEN, 2, 0, ref.NOSOLN), (16, ref.EMPTY_TRANSITION, 2, 65, ref.NOSOLN),
    (8, ref.NO_STOPBAND_A, 2, 10, ref.UNKNOWN), (8, ref.NO_STOPBAND_B, 2, 10, ref.UNKNOWN)])
def test_pinned_runs(gpu, n, consts, B, niter, status):
    recs = check_optim(gpu, n, [consts] * B)
    assert recs[0]["niter"] == niter and recs[0]["status"] == status


def test_no_stopband_pair_in_one_batch(gpu):
    check_optim(gpu, 8, [ref.NO_STOPBAND_A, ref.NO_STOPBAND_B])


# ---- 4. a mixed sweep -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(16, 37), (32, 12)])
def test_mixed_sweep(gpu, n, B):
    consts = [ref.family(s) for s in range(B)]
    recs = [ref.solve_optim(n, c) for c in consts]
    assert all(r["x_best"] is not None and r["niter"] < MAX_ITERS for r in recs)
    assert len({r["niter"] for r in recs}) > 1
    check_optim(gpu, n, consts)


# ---- 5. shapes where the mapping can go wrong -------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(1, 70), (2, 5), (3, 67), (7, 5), (33, 4), (65, 2)])
def test_odd_sizes_on_the_loose_set(gpu, n, B):
    check_optim(gpu, n, [ref.LOOSE] * B)


def test_n128_cut_off(gpu):
    recs = check_optim(gpu, 128, [ref.LOOSE] * 3, max_iters=300)
    assert recs[0]["niter"] == 300 and recs[0]["status"] == ref.SUCCESS


def test_stops_at_zero_and_unknown_beside_a_live_instance(gpu):
    recs = check_optim(gpu, 8, [ref.AS_WRITTEN, ref.NO_STOPBAND_B, ref.LOOSE, ref.NO_STOPBAND_A, ref.LOOSE])
    assert [r["status"] for r in recs[:2]] == [ref.NOSOLN, ref.UNKNOWN] and recs[0]["niter"] == 0
    assert recs[2]["niter"] > recs[1]["niter"]


# ---- 6. chunking ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunking_changes_nothing(gpu, chunk):
    check_optim(gpu, 16, [ref.family(s) for s in range(37)], chunk=chunk)


# ---- 7. cut-off and resume --------------------------------------------------------------------------------------------
def test_cut_off_and_resume_and_reset(gpu):
    n, B = 16, 12
    consts = [ref.family(s) for s in range(B)]
    gamma0 = np.array([c[4] for c in consts])
    full = [ref.solve_optim(n, c) for c in consts]
    first, second, spaces, omegas = [], [], [], []
    for c in consts:
        omega, space = ref.fresh(n, c)
        xb, niter, gamma, status = omega.cutting_plane_optim(space, c[4], 100, TOL)
        first.append(dict(x_best=xb, niter=niter, gamma=gamma, status=status, state=omega.state(), **ref.space_record(space)))
        spaces.append(space)
        omegas.append(omega)
    assert all(r["niter"] == 100 for r in first)
    prob, batch = make_gpu(gpu, n, consts)
    got = prob.optim(batch, gamma0, 100, TOL)
    assert_runs_equal(got, first, n)
    assert_state_equal(prob, [r["state"] for r in first])
    assert_spaces_equal(batch, first)
    for r, space, omega in zip(first, spaces, omegas):
        xb, niter, gamma, status = omega.cutting_plane_optim(space, r["gamma"], MAX_ITERS - 100, TOL)
        second.append(dict(x_best=xb, niter=niter, gamma=gamma, status=status, state=omega.state(), **ref.space_record(space)))
    for r, f in zip(second, full):  # the CPU run driven this way is the uninterrupted run
        assert r["niter"] + 100 == f["niter"] and r["gamma"] == f["gamma"] and r["state"] == f["state"]
        assert r["x_best"] is not None and np.array_equal(r["x_best"], f["x_best"]) and np.array_equal(r["mq"], f["mq"])
    got2 = prob.optim(batch, got[3], MAX_ITERS - 100, TOL)
    assert_runs_equal(got2, second, n)
    assert_state_equal(prob, [r["state"] for r in second])
    assert_spaces_equal(batch, second)
    # reset: cursors, fmax and kmax as after new(); a rerun from fresh spaces reproduces the whole run
    prob.reset()
    s = prob.state()
    np.testing.assert_array_equal(s["idx1"], np.full(B, -1))
    np.testing.assert_array_equal(s["idx2"], s["nwpass"] - 1)
    np.testing.assert_array_equal(s["idx3"], s["nwstop"] - 1)
    np.testing.assert_array_equal(s["kmax"], np.full(B, -1))
    assert (s["fmax"] == -np.inf).all() and (s["more_alt"] == 1).all()
    batch = gpu.EllBatch.new_with_scalar(np.full(B, ref.KAPPA), np.zeros((B, n)))
    assert_runs_equal(prob.optim(batch, gamma0, MAX_ITERS, TOL), full, n)
    assert_state_equal(prob, [r["state"] for r in full])
    assert_spaces_equal(batch, full)


def test_max_iters_zero_moves_nothing(gpu):
    n, consts = 16, [ref.family(s) for s in range(5)]
    prob, batch = make_gpu(gpu, n, consts)
    before = (batch.mq, batch.xc(), batch.kappa, prob.state())
    x_best, has, niter, gamma, status = prob.optim(batch, 0.05, 0, TOL)
    assert (niter == 0).all() and (has == 0).all() and (status == ref.SUCCESS).all() and np.isnan(x_best).all()
    assert (gamma == 0.05).all()
    after = (batch.mq, batch.xc(), batch.kappa, prob.state())
    for a, b in zip(before[:3], after[:3]):
        np.testing.assert_array_equal(a, b)
    for k in ref.STATE_KEYS:
        np.testing.assert_array_equal(before[3][k], after[3][k])


# ---- 8. feasibility ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,consts,B,feasible,niter", [(16, ref.LOOSE, 3, True, 17), (32, ref.CORRECTED, 2, True, 69),
                                                       (32, ref.FEAS_INFEASIBLE, 2, False, 187)])
def test_feas_pins(gpu, n, consts, B, feasible, niter):
    recs = check_feas(gpu, n, [consts] * B)
    assert (recs[0]["x_best"] is not None) == feasible and recs[0]["niter"] == niter
    assert recs[0]["status"] == (ref.SUCCESS if feasible else ref.NOSOLN)


def test_feas_mixed_batch(gpu):
    consts = [ref.CORRECTED, ref.FEAS_INFEASIBLE, ref.LOOSE, ref.FEAS_INFEASIBLE, ref.AS_WRITTEN, ref.SHORT_PASSBAND,
              ref.CORRECTED, ref.LOOSE, ref.FEAS_INFEASIBLE]
    recs = check_feas(gpu, 32, consts)
    assert {r["x_best"] is not None for r in recs} == {True, False}


# ---- 9. interleaving with the batch engine ----------------------------------------------------------------------------
def test_batch_update_between_two_loops(gpu):
    n, B = 16, 12
    consts = [ref.family(s) for s in range(B)]
    prob, batch = make_gpu(gpu, n, consts)
    pairs = [ref.fresh(n, c) for c in consts]
    first = []
    for (omega, space), c in zip(pairs, consts):
        xb, niter, gamma, status = omega.cutting_plane_optim(space, c[4], 60, TOL)
        first.append(dict(x_best=xb, niter=niter, gamma=gamma, status=status, **ref.space_record(space)))
    got = prob.optim(batch, np.array([c[4] for c in consts]), 60, TOL)
    assert_runs_equal(got, first, n)
    rng = np.random.default_rng(3)
    grads = rng.standard_normal((1, B, n))
    kinds = rng.integers(0, 2, size=(1, B)).astype(np.int32)
    beta = np.zeros((1, B))
    want = np.zeros((1, B), dtype=np.int32)
    for b, (omega, space) in enumerate(pairs):
        beta[0, b] = 0.1 * np.sqrt(space.tsq) if kinds[0, b] == 0 else 0.0
        want[0, b] = space.update(int(kinds[0, b]), grads[0, b], beta[0, b])
    status, _ = batch.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    assert_spaces_equal(batch, [ref.space_record(space) for _, space in pairs])
    second = []
    for (omega, space), r in zip(pairs, first):
        xb, niter, gamma, status = omega.cutting_plane_optim(space, r["gamma"], MAX_ITERS, TOL)
        second.append(dict(x_best=xb, niter=niter, gamma=gamma, status=status, **ref.space_record(space)))
    assert all(r["niter"] < MAX_ITERS for r in second)
    assert_runs_equal(prob.optim(batch, got[3], MAX_ITERS, TOL), second, n)
    assert_state_equal(prob, [omega.state() for omega, _ in pairs])
    assert_spaces_equal(batch, second)


# ---- 10. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_spaces_untouched(gpu):
    lib = gpu.capi.load()
    n, B = 8, 4
    prob = gpu.BatchLowpassProblem(n, *ref.columns([ref.LOOSE] * B))
    rng = np.random.default_rng(2)

    def refused(batch, entry="optim"):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        gamma = np.full(batch.B, 0.3)
        xb = np.full((batch.B, batch.n), np.nan)
        has = np.zeros(batch.B, dtype=np.int32)
        niter = np.zeros(batch.B, dtype=np.int64)
        status = np.zeros(batch.B, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        if entry == "optim":
            rc = lib.ellhip_batch_lowpass_optim(batch._h, prob._h, ptr(gamma), 100, 1e-10, ptr(xb), ptr(has), ptr(niter),
                                                ptr(status))
        else:
            rc = lib.ellhip_batch_lowpass_feas(batch._h, prob._h, 100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status))
        assert rc == gpu.capi.E_INVALID and lib.ellhip_last_error()
        for a, b in zip(before, (batch.mq, batch.xc(), batch.kappa, batch.tsq())):
            np.testing.assert_array_equal(a, b)
        assert np.isnan(xb).all()

    stable = gpu.EllStableBatch.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n)))
    refused(stable)
    refused(stable, "feas")
    refused(gpu.EllBatch.new_with_scalar(np.full(B + 1, 10.0), rng.standard_normal((B + 1, n))))   # wrong B
    refused(gpu.EllBatch.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n + 1))))       # wrong n
    with pytest.raises(gpu.capi.EllHipError, match="wpass > wstop"):
        gpu.BatchLowpassProblem(n, [0.1, 0.3], [0.2, 0.2], 0.5, 1.5, 0.3)
    with pytest.raises(gpu.capi.EllHipError):
        gpu.BatchLowpassProblem(129, *ref.columns([ref.LOOSE]))
    with pytest.raises(gpu.capi.EllHipError):
        gpu.BatchLowpassProblem(0, *ref.columns([ref.LOOSE]))
    with pytest.raises(gpu.capi.EllHipError):
        prob.set_chunk(0)
    with pytest.raises(gpu.capi.EllHipError):
        prob.set_chunk(4097)
    with pytest.raises(ValueError):
        prob.assess_feas(np.zeros((B, n + 1)))
    # and a good pair still runs
    good = gpu.EllBatch.new_with_scalar(np.full(B, ref.KAPPA), np.zeros((B, n)))
    assert (prob.optim(good, 0.3, 5, TOL)[2] <= 5).all()


def test_caller_supplied_spectrum(gpu, orc):
    n = 16
    cpu_o = orc.OracleLowpass(n, *ref.LOOSE)
    spec = cpu_o.spectrum.copy()
    spec[5] *= 1.5  # not the computed table any more
    prob = gpu.BatchLowpassProblem(n, *ref.columns([ref.LOOSE] * 2), spectrum=spec)
    np.testing.assert_array_equal(prob.spectrum, spec)


# ---- 11. the C++ mirror -----------------------------------------------------------------------------------------------
def test_cpp_runner_matches_the_cpu_runs(gpu):
    import cpp_build
    exe = cpp_build.build_runner("batch_lowpass_runner.cpp", "hip")
    got = cpp_build.run_json_lines(exe)
    n, B = 16, 37
    assert len(got) == B
    for b in range(B):
        d, r = got[f"sweep_{b}"], ref.solve_optim(n, ref.family(b))
        assert d["niter"] == r["niter"] and d["status"] == r["status"] and d["has_best"] == 1
        assert d["gamma"] == r["gamma"] and d["x_best"] == r["x_best"].tolist()
        assert (d["idx1"], d["idx2"], d["idx3"], d["kmax"]) == tuple(r["state"][k] for k in ("idx1", "idx2", "idx3", "kmax"))
