"""GPU: the batched device-resident LMI cutting-plane loop (include/ellhip_batch_lmi.h) against the CPU restatement
(tests/batch_lmi_reference.py over the CPU oracle).  Oracle and update follow the reference's fold order, so every
comparison is EXACT: == on float64 bits and on integers -- x_best, has_best, niter, gamma, status, idx and the spaces' xc,
Q, kappa and tsq afterwards."""
import ctypes as C
import math

import numpy as np
import pytest

import batch_lmi_reference as ref

pytestmark = pytest.mark.gpu

FAMILY_B = [(8, 6, 2, 1e-10), (16, 12, 3, 1e-8), (32, 24, 2, 1e-6)]


def make_gpu(gpu, problems, *, lmi0=False, with_c=True, kappa=10.0, xc0=None):
    mat_f, mat_b, c = ref.stack(problems)
    B, n = c.shape
    prob = gpu.BatchLmiProblem(mat_f, None if lmi0 else mat_b, c if with_c else None)
    batch = gpu.EllBatch.new_with_scalar(np.full(B, kappa), np.zeros((B, n)) if xc0 is None else xc0)
    return prob, batch


def assert_spaces_equal(batch, spaces):
    np.testing.assert_array_equal(batch.mq, np.stack([np.array(s.mq) for s in spaces]))
    np.testing.assert_array_equal(batch.xc(), np.stack([np.array(s.xc) for s in spaces]))
    np.testing.assert_array_equal(batch.kappa, np.array([s.kappa for s in spaces]))
    np.testing.assert_array_equal(batch.tsq(), np.array([s.tsq for s in spaces]))


def assert_runs_equal(got, runs, omegas, prob):
    x_best, has, niter, gamma, status = got
    np.testing.assert_array_equal(niter, np.array([r["niter"] for r in runs], dtype=np.int64))
    np.testing.assert_array_equal(status, np.array([r["status"] for r in runs], dtype=np.int32))
    np.testing.assert_array_equal(gamma, np.array([r["gamma"] for r in runs]))
    np.testing.assert_array_equal(has, np.array([r["x_best"] is not None for r in runs], dtype=np.int32))
    n = x_best.shape[1]
    want = np.stack([np.full(n, np.nan) if r["x_best"] is None else r["x_best"] for r in runs])
    np.testing.assert_array_equal(x_best, want)  # rows without a best point stay as the caller left them (NaN)
    np.testing.assert_array_equal(prob.idx, np.array([o.idx for o in omegas], dtype=np.int32))


def check_optim(gpu, problems, max_iters, tol, *, lmi0=False, chunk=None, require_best=True):
    runs, spaces, omegas = ref.run_optim(problems, max_iters, tol, lmi0=lmi0)
    if require_best:  # the families' condition, asserted on the CPU side before comparing
        assert all(r["niter"] < max_iters and r["x_best"] is not None for r in runs)
    prob, batch = make_gpu(gpu, problems, lmi0=lmi0)
    if chunk is not None:
        prob.set_chunk(chunk)
    got = prob.optim(batch, math.inf, max_iters, tol)
    assert_runs_equal(got, runs, omegas, prob)
    assert_spaces_equal(batch, spaces)
    return runs


# ---- 1. the oracle alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["A", "B8", "B16"])
def test_assess_optim_call_by_call(gpu, family):
    if family == "A":
        problems = [ref.family_a(s) for s in range(64)]
    elif family == "B8":
        problems = [ref.family_b(s, 8, 6, 2) for s in range(16)]
    else:
        problems = [ref.family_b(s, 16, 12, 3) for s in range(16)]
    B, n, J = len(problems), len(problems[0][2]), len(problems[0][0])
    mat_f, mat_b, c = ref.stack(problems)
    prob = gpu.BatchLmiProblem(mat_f, mat_b, c)
    omegas = [ref.RoundRobinLmi(fs, bs, cc) for fs, bs, cc in problems]
    np.testing.assert_array_equal(prob.idx, np.full(B, -1, dtype=np.int32))
    rng = np.random.default_rng(17)
    gamma = np.full(B, math.inf)
    seen = set()
    for call in range(10):
        # near 0 every block passes (B_j > 0); farther out the blocks cut; a repeated point meets the objective cut
        scale = rng.choice([0.0, 0.02, 0.3, 3.0], size=(B, 1))
        x = scale * rng.standard_normal((B, n))
        grad, beta, station, gamma_out = prob.assess_optim(x, gamma)
        for b in range(B):
            (g, be), st, ga = omegas[b].assess_optim(x[b], gamma[b])
            assert station[b] == st and beta[b] == be and gamma_out[b] == ga, (call, b)
            np.testing.assert_array_equal(grad[b], g)
            seen.add(st)
        np.testing.assert_array_equal(prob.idx, np.array([o.idx for o in omegas], dtype=np.int32))
        gamma = gamma_out
    assert J in seen and J + 1 in seen and any(s < J for s in seen)  # objective cut, shrunk, block cuts
    prob.idx = None
    np.testing.assert_array_equal(prob.idx, np.full(B, -1, dtype=np.int32))


# ---- 2. the reference problem ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 257])
def test_reference_problem_copies(gpu, B):
    runs = check_optim(gpu, [ref.reference_problem()] * B, 2000, 1e-20)
    assert runs[0]["niter"] == 11 and runs[0]["status"] == ref.NOSOLN and runs[0]["gamma"] == -3.7502205782089257


# ---- 3. the families -------------------------------------------------------------------------------------------------
def test_family_a(gpu):
    runs = check_optim(gpu, [ref.family_a(s) for s in range(64)], 2000, 1e-20)
    assert len({r["niter"] for r in runs}) > 1  # instances stop at different iterations


@pytest.mark.parametrize("n,m,J,tol", FAMILY_B)
def test_family_b(gpu, n, m, J, tol):
    runs = check_optim(gpu, [ref.family_b(s, n, m, J) for s in range(16)], 2000, tol)
    assert all(r["status"] == ref.SUCCESS for r in runs)


def test_single_block_handle(gpu):
    check_optim(gpu, [ref.family_b(s, 8, 6, 1) for s in range(16)], 2000, 1e-10)


def test_n128_with_small_blocks_fits(gpu):
    check_optim(gpu, [ref.family_b(s, 128, 8, 2) for s in range(3)], 40, 1e-10, require_best=False)


def test_lmi0_form(gpu):
    # sum_k x_k F_k > 0 with random F: most likely empty, the loop ends where the CPU's does
    check_optim(gpu, [ref.family_b(s, 8, 6, 2) for s in range(16)], 300, 1e-10, lmi0=True, require_best=False)
    # with F_0 positive definite the cone is not empty (x = e_0)
    problems = []
    for s in range(16):
        fs, bs, c = ref.family_b(s, 8, 6, 2)
        for f, b in zip(fs, bs):
            f[0] = b
        problems.append((fs, bs, c))
    runs = check_optim(gpu, problems, 300, 1e-10, lmi0=True, require_best=False)
    assert any(r["x_best"] is not None for r in runs)


# ---- 4. chunking -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunking_changes_nothing(gpu, chunk):
    check_optim(gpu, [ref.family_a(s) for s in range(64)], 2000, 1e-20, chunk=chunk)
    check_optim(gpu, [ref.family_b(s, 8, 6, 2) for s in range(16)], 2000, 1e-10, chunk=chunk)


# ---- 5. cut-off and resume -------------------------------------------------------------------------------------------
def test_cut_off_and_resume(gpu):
    problems = [ref.family_b(s, 8, 6, 2) for s in range(16)]
    runs, spaces, omegas = ref.run_optim(problems, 50, 1e-10)
    assert all(r["niter"] == 50 for r in runs)
    prob, batch = make_gpu(gpu, problems)
    got = prob.optim(batch, math.inf, 50, 1e-10)
    assert (got[2] == 50).all()
    assert_runs_equal(got, runs, omegas, prob)
    assert_spaces_equal(batch, spaces)
    # max_iters = 0: nothing moves
    got0 = prob.optim(batch, got[3], 0, 1e-10)
    assert (got0[2] == 0).all() and (got0[1] == 0).all() and (got0[4] == ref.SUCCESS).all() and np.isnan(got0[0]).all()
    np.testing.assert_array_equal(got0[3], got[3])
    assert_spaces_equal(batch, spaces)
    np.testing.assert_array_equal(prob.idx, np.array([o.idx for o in omegas], dtype=np.int32))
    # the second call: idx and gamma carry over, x_best starts empty
    runs2 = []
    for r, space, omega in zip(runs, spaces, omegas):
        x_best, niter, gamma, status = ref.optim(space, omega, r["gamma"], 2000, 1e-10)
        runs2.append(dict(x_best=x_best, niter=niter, gamma=gamma, status=status))
    assert all(r["niter"] < 2000 for r in runs2)
    got2 = prob.optim(batch, got[3], 2000, 1e-10)
    assert_runs_equal(got2, runs2, omegas, prob)
    assert_spaces_equal(batch, spaces)


# ---- 6. interoperation with the batch engine ---------------------------------------------------------------------------
def test_batch_update_continues_from_the_loop(gpu):
    problems = [ref.family_b(s, 8, 6, 2) for s in range(16)]
    runs, spaces, omegas = ref.run_optim(problems, 60, 1e-10)
    prob, batch = make_gpu(gpu, problems)
    assert_runs_equal(prob.optim(batch, math.inf, 60, 1e-10), runs, omegas, prob)
    rng = np.random.default_rng(3)
    K, B, n = 3, 16, 8
    grads = rng.standard_normal((K, B, n))
    kinds = rng.integers(0, 2, size=(K, B)).astype(np.int32)
    beta = np.zeros((K, B))
    want = np.zeros((K, B), dtype=np.int32)
    for k in range(K):
        for b in range(B):
            beta[k, b] = 0.1 * math.sqrt(spaces[b].tsq) if kinds[k, b] == 0 else 0.0
            want[k, b] = spaces[b].update(int(kinds[k, b]), grads[k, b], beta[k, b])
    status, _ = batch.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    assert_spaces_equal(batch, spaces)


def test_spaces_from_one_handle_are_loop_input(gpu):
    B = 9
    problems = [ref.family_a(s) for s in range(B)]
    runs, spaces, omegas = ref.run_optim(problems, 2000, 1e-20)
    mat_f, mat_b, c = ref.stack(problems)
    prob = gpu.BatchLmiProblem(mat_f, mat_b, c)
    batch = gpu.EllBatch.from_space(gpu.Ell.new_with_scalar(10.0, np.zeros(3)), B)
    assert_runs_equal(prob.optim(batch, math.inf, 2000, 1e-20), runs, omegas, prob)
    assert_spaces_equal(batch, spaces)


# ---- 7. feasibility problems -----------------------------------------------------------------------------------------
def check_feas(gpu, problems, max_iters, tol, *, lmi0=False, kappa=100.0, seed=11, zero_start=False):
    B, n = len(problems), len(problems[0][2])
    xc0 = 3.0 * np.random.default_rng(seed).standard_normal((B, n))
    if zero_start:  # instance 0 starts where the reference's own runs start; the random rows are as without it
        xc0 = np.vstack([np.zeros((1, n)), xc0[:B - 1]])
    want = []
    spaces, omegas = [], []
    for b, (fs, bs, _) in enumerate(problems):
        space = ref.O.OracleEll.new_with_scalar(kappa, xc0[b])
        omega = ref.RoundRobinLmi(fs, None if lmi0 else bs, None)
        want.append(ref.feas(space, omega, max_iters, tol))
        spaces.append(space)
        omegas.append(omega)
    prob, batch = make_gpu(gpu, problems, lmi0=lmi0, with_c=False, kappa=kappa, xc0=xc0)
    x, ok, niter, status = prob.feas(batch, max_iters, tol)
    np.testing.assert_array_equal(niter, np.array([w[1] for w in want], dtype=np.int64))
    np.testing.assert_array_equal(status, np.array([w[2] for w in want], dtype=np.int32))
    np.testing.assert_array_equal(ok, np.array([w[0] is not None for w in want], dtype=np.int32))
    np.testing.assert_array_equal(x, np.stack([np.full(n, np.nan) if w[0] is None else w[0] for w in want]))
    np.testing.assert_array_equal(prob.idx, np.array([o.idx for o in omegas], dtype=np.int32))
    assert_spaces_equal(batch, spaces)
    return want


def test_feas_families(gpu):
    want = check_feas(gpu, [ref.family_a(s) for s in range(64)], 2000, 1e-20)
    assert any(w[0] is not None and w[1] > 0 for w in want)  # feasible points found after some cuts
    want = check_feas(gpu, [ref.family_b(s, 8, 6, 2) for s in range(16)], 2000, 1e-10)
    assert any(w[0] is not None and w[1] > 0 for w in want)
    check_feas(gpu, [ref.family_b(s, 16, 12, 3) for s in range(16)], 2000, 1e-8)


def test_feas_lmi0_form_of_f1(gpu):
    """The LMI0 form of the reference's F1 alone (tests/lmi_tests.rs:65-71: it cuts at x = 0), 200 iterations at most, ends
    exactly as the CPU does.  The three matrices of F1 span the symmetric 2 x 2 matrices, so sum_k x_k F1_k > 0 has
    solutions and the CPU loop finds one: from Ell::new_with_scalar(10, 0) after 1 iteration
    (x = (-0.54794625, 0.54794625, -0.15655607)), from the five random starts used here after 2, 6, 0 and 3 iterations, and
    one start ends NoSoln after 2.  It is therefore not an infeasible handle; the device must still reproduce every one of
    these endings bit for bit, and the infeasible case proper is the next test."""
    fs, bs, c = ref.reference_problem()
    want = check_feas(gpu, [([fs[0]], [bs[0]], c)] * 6, 200, 1e-20, lmi0=True, kappa=10.0, zero_start=True)
    assert want[0][0] is not None and want[0][1] == 1 and want[0][2] == ref.SUCCESS
    assert any(w[0] is None and w[2] == ref.NOSOLN for w in want)


def test_feas_infeasible_handle(gpu):
    """An LMI0 handle with no solution: three traceless matrices (every combination has trace 0, so none is positive
    definite).  Every instance must end NoSoln or at max_iters, exactly as the CPU does (there: NoSoln after 0 to 64
    iterations, with tsq down at the rounding level of either sign before the end)."""
    t = np.array([[[1.0, 0.0], [0.0, -1.0]], [[0.0, 1.0], [1.0, 0.0]], [[2.0, 3.0], [3.0, -2.0]]])
    want = check_feas(gpu, [([t], [np.eye(2)], np.ones(3))] * 6, 200, 1e-20, lmi0=True, kappa=10.0, zero_start=True)
    assert all(w[0] is None and (w[2] == ref.NOSOLN or w[1] == 200) for w in want)
    assert max(w[1] for w in want) > 10


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_spaces_untouched(gpu):
    lib = gpu.capi.load()
    problems = [ref.family_a(s) for s in range(4)]
    mat_f, mat_b, c = ref.stack(problems)
    prob = gpu.BatchLmiProblem(mat_f, mat_b, c)
    prob_feas = gpu.BatchLmiProblem(mat_f, mat_b, None)
    rng = np.random.default_rng(2)

    def refused(batch, p, entry="optim"):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        B, n = batch.B, batch.n
        gamma = np.full(B, math.inf)
        xb = np.full((B, n), np.nan)
        has = np.zeros(B, dtype=np.int32)
        niter = np.zeros(B, dtype=np.int64)
        status = np.zeros(B, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        if entry == "optim":
            rc = lib.ellhip_batch_lmi_optim(batch._h, p._h, ptr(gamma), 100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status))
        else:
            rc = lib.ellhip_batch_lmi_feas(batch._h, p._h, 100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status))
        assert rc == gpu.capi.E_INVALID and lib.ellhip_last_error()
        after = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        for a, b in zip(before, after):
            np.testing.assert_array_equal(a, b)
        assert np.isnan(xb).all()

    refused(gpu.EllStableBatch.new_with_scalar(np.full(4, 10.0), rng.standard_normal((4, 3))), prob)
    refused(gpu.EllBatch.new_with_scalar(np.full(5, 10.0), rng.standard_normal((5, 3))), prob)   # wrong B
    refused(gpu.EllBatch.new_with_scalar(np.full(4, 10.0), rng.standard_normal((4, 4))), prob)   # wrong n
    good = gpu.EllBatch.new_with_scalar(np.full(4, 10.0), rng.standard_normal((4, 3)))
    refused(good, prob_feas)             # _optim on a handle made without c
    refused(good, prob, entry="feas")    # _feas on a handle made with c
    # a shape that needs more LDS than a workgroup has: n = 128 with a 64 x 64 block
    big = gpu.BatchLmiProblem([np.zeros((1, 128, 64, 64))], [np.eye(64)[None]], np.ones((1, 128)))
    refused(gpu.EllBatch.new_with_scalar(np.full(1, 10.0), np.zeros((1, 128))), big)
    # shapes refused at creation
    flat_f = np.concatenate([f.ravel() for f in mat_f])
    flat_b = np.concatenate([b.ravel() for b in mat_b])
    h = C.c_void_p()
    for J, m in ((0, [2, 3]), (9, [2] * 9), (2, [2, 65])):
        m = np.array(m, dtype=np.int64)
        rc = lib.ellhip_batch_lmi_create(C.byref(h), 4, 3, J, m.ctypes.data, flat_f.ctypes.data, flat_b.ctypes.data,
                                         c.ctypes.data, -1)
        assert rc == gpu.capi.E_INVALID and not h.value
    with pytest.raises(gpu.capi.EllHipError):
        prob.set_chunk(0)
    with pytest.raises(gpu.capi.EllHipError):
        prob.set_chunk(4097)
    # and the good pair still runs
    x_best, has, niter, gamma, status = prob.optim(good, math.inf, 5, 1e-20)
    assert (niter <= 5).all()


# ---- 9. the C++ mirror -----------------------------------------------------------------------------------------------
def test_cpp_runner_matches_the_python_path(gpu):
    import cpp_build
    exe = cpp_build.build_runner("batch_lmi_runner.cpp", "hip")
    got = cpp_build.run_json_lines(exe)
    B = 37
    prob, batch = make_gpu(gpu, [ref.reference_problem()] * B)
    x_best, has, niter, gamma, status = prob.optim(batch, math.inf, 2000, 1e-20)
    assert len(got) == B
    for b in range(B):
        d = got[f"ref_{b}"]
        assert d["niter"] == niter[b] and d["status"] == status[b] and d["has_best"] == has[b]
        assert d["gamma"] == gamma[b]
        assert d["x_best"] == x_best[b].tolist()
    assert niter[0] == 11 and gamma[0] == -3.7502205782089257
