"""GPU: the batched device-resident SVM loop (include/ellhip_batch_svm.h) against the reference's SvmOracle restated in
tests/svm_reference.py and its cutting_plane_optim over the CPU oracle's Ell (tests/batch_svm_reference.py).  The device
folds every margin like the CPU and picks the sample by the reference's scan rule, so every comparison is EXACT: float64
bit patterns (the sign of a zero counts; NaN is compared by position) and integers -- margins, gradient, beta, gamma,
min_idx / min_val, x_best, has_best, niter, status and the spaces' Q, xc, kappa and tsq afterwards."""
import ctypes as C
import struct

import numpy as np
import pytest

import batch_svm_reference as ref
import svm_reference as svm

pytestmark = pytest.mark.gpu

INF = np.inf
LABELS = np.array([-7, -1, 0, 1, 7], dtype=np.int32)
# (m, nfeat, B): smallest shape; n = 2 with a partial last workgroup; m < n; n = 3 does not divide 64; n = 17 straddles
# waves; n = 64; n = 65 (one instance per workgroup); n = 128
SHAPES = [(1, 1, 70), (5, 1, 70), (3, 7, 5), (64, 2, 67), (97, 16, 5), (130, 63, 3), (67, 64, 2), (130, 127, 2)]


def same_bits(a, b):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def assert_bits(got, want, what):
    assert same_bits(got, want), (what, got, want)


def new_batch(gpu, B, n):
    return gpu.EllBatch.new_with_scalar(np.full(B, ref.KAPPA), np.zeros((B, n)))


def table(data, b):
    return data if data.ndim == 2 else data[b]


# ---- 1. the oracle call by call ---------------------------------------------------------------------------------------
def check_calls(prob, data, lab, x):
    """margins, assess_optim and last of every problem at x [B][n] against svm_reference"""
    B = lab.shape[0]
    mg = prob.margins(x)
    before = prob.last()
    grad, beta, gamma = prob.assess_optim(x)
    idx, val = prob.last()
    for b in range(B):
        X = table(data, b)
        assert_bits(mg[b], svm.margins(X, lab[b], x[b]), f"margins {b}")
        (rg, rb), _, rgamma, ridx, rval = svm.assess_optim(X, lab[b], x[b])
        assert idx[b] == ridx and same_bits(val[b], rval), (b, idx[b], val[b], ridx, rval)
        assert_bits(grad[b], rg, f"grad {b}")
        assert same_bits(beta[b], rb) and same_bits(gamma[b], rgamma), (b, beta[b], gamma[b], rb, rgamma)
    return before, (idx, val)


@pytest.mark.parametrize("m,nfeat,B", SHAPES)
def test_oracle_call_by_call(gpu, m, nfeat, B):
    rng = np.random.default_rng(1000 * m + nfeat)
    data = rng.standard_normal((B, m, nfeat))
    lab = rng.choice(LABELS, size=(B, m))
    per = gpu.BatchSvmProblem(data, lab)
    shared = gpu.BatchSvmProblem(data[B - 1], lab)
    assert per.n == nfeat + 1 and not per.shared and shared.shared
    idx, val = per.last()   # as after new(): nothing scanned yet
    assert not idx.any() and (val == INF).all()
    for _ in range(2):
        x = rng.standard_normal((B, nfeat + 1))
        check_calls(per, data, lab, x)
        check_calls(shared, data[B - 1], lab, x)
    # margins() looks without touching what last() reports
    kept = per.last()
    per.margins(rng.standard_normal((B, nfeat + 1)))
    assert np.array_equal(per.last()[0], kept[0]) and same_bits(per.last()[1], kept[1])


def test_margins_special_values(gpu):
    m, nfeat, B = 97, 16, 5
    rng = np.random.default_rng(5)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-310, -2.5])
    data = rng.choice(specials, size=(B, m, nfeat), p=[0.2, 0.2, 0.03, 0.03, 0.02, 0.2, 0.2, 0.05, 0.07])
    lab = rng.choice(LABELS, size=(B, m))
    prob = gpu.BatchSvmProblem(data, lab)
    n = nfeat + 1
    for x in (np.zeros(n), np.full(n, -0.0), rng.choice(specials[[0, 1, 5, 6, 8]], size=n),
              np.where(rng.random(n) < 0.5, -0.0, 0.0)):
        xs = np.tile(x, (B, 1))
        check_calls(prob, data, lab, xs)
        mg = prob.margins(xs)
        assert np.isnan(mg).any() and (mg == 0).any()


def test_margins_equal_the_single_problem_oracle(gpu):
    m, nfeat, B = 130, 63, 3
    rng = np.random.default_rng(8)
    data = rng.standard_normal((B, m, nfeat))
    lab = rng.choice(LABELS, size=(B, m))
    x = rng.standard_normal((B, nfeat + 1))
    mg = gpu.BatchSvmProblem(data, lab).margins(x)
    for b in range(B):
        assert_bits(mg[b], gpu.SvmOracle(data[b], lab[b]).margins(x[b]), f"problem {b}")


# ---- 2. ties ----------------------------------------------------------------------------------------------------------
def test_duplicate_rows_first_index_wins(gpu):
    m, nfeat, B = 64, 2, 3
    rng = np.random.default_rng(3)
    data = rng.standard_normal((B, m, nfeat))
    lab = np.ones((B, m), dtype=np.int32)
    x = rng.standard_normal((B, nfeat + 1))
    want = []
    for b in range(B):
        r = svm.argmin(svm.margins(data[b], lab[b], x[b]))[0]
        dup = [(r + 7) % m, (r + 30) % m, (r + 32) % m]   # later copies, in other threads' strides and in the winner's own
        data[b, dup] = data[b, r]
        want.append(min([r] + dup))
    prob = gpu.BatchSvmProblem(data, lab)
    check_calls(prob, data, lab, x)
    assert prob.last()[0].tolist() == want


@pytest.mark.parametrize("second", [6, 7])   # index 6: thread 0 holds the later zero; index 7: both in thread 1's stride
def test_signed_zero_ties_keep_the_first_index_and_its_sign(gpu, second):
    """n = 3: every margin is 5 except indices 4 and `second`, zeros of opposite sign, in both orders (problems 0 and 1).
    The earlier index belongs to the higher-numbered thread when second = 6."""
    m = 9
    data = np.zeros((m, 2))
    data[:, 0] = 5.0
    data[4, 0] = data[second, 0] = 0.0
    lab = np.ones((2, m), dtype=np.int32)
    lab[0, 4], lab[0, second] = -1, 1
    lab[1, 4], lab[1, second] = 1, -1
    prob = gpu.BatchSvmProblem(data, lab)     # one shared table, the labels differ
    x = np.tile([1.0, 0.0, 0.0], (2, 1))
    check_calls(prob, data, lab, x)
    idx, val = prob.last()
    assert idx.tolist() == [4, 4] and (val == 0.0).all()
    assert np.signbit(val).tolist() == [True, False]
    grad, beta, gamma = prob.assess_optim(x)
    assert np.signbit(beta).tolist() == [True, False] and np.signbit(gamma).tolist() == [True, False]


def test_zero_cut_and_infinite_margins(gpu):
    m, nfeat, B = 64, 6, 4
    sets = [ref.clouds(m, nfeat, 1.0, s) for s in range(B)]
    data = np.stack([X for X, _ in sets])
    lab = np.stack([l for _, l in sets])
    prob = gpu.BatchSvmProblem(data, lab)
    n = nfeat + 1
    # an all-NaN x: every margin is NaN, nothing is below +inf -> (0, +inf), the zero cut, gamma = +0.0
    grad, beta, gamma = prob.assess_optim(np.full((B, n), np.nan))
    assert_bits(grad, np.zeros((B, n)), "grad")
    assert_bits(beta, np.zeros(B), "beta")
    assert_bits(gamma, np.zeros(B), "gamma")
    idx, val = prob.last()
    assert not idx.any() and (val == INF).all()
    # a separating point: min_val >= 1 -> the zero cut, and last() still reports the scan
    x = np.zeros((B, n))
    x[:, 0] = 4.0
    _, (idx, val) = check_calls(prob, data, lab, x)
    grad, beta, gamma = prob.assess_optim(x)
    assert (val >= 1.0).all() and not grad.any() and same_bits(gamma, np.zeros(B))
    # a -inf margin at two indices: the first wins, the gradient carries the infinity
    data2, lab2 = data.copy(), lab.copy()
    data2[:, 40, 0] = data2[:, 10, 0] = -np.inf
    lab2[:, 40] = lab2[:, 10] = 1
    prob2 = gpu.BatchSvmProblem(data2, lab2)
    _, (idx, val) = check_calls(prob2, data2, lab2, x)
    grad, _, gamma = prob2.assess_optim(x)
    assert (idx == 10).all() and (val == -INF).all() and (grad[:, 0] == INF).all() and (gamma == -INF).all()


# ---- 3. loops against the CPU runs ------------------------------------------------------------------------------------
def assert_runs_equal(got, recs, n):
    x_best, has, niter, gamma, status = got
    np.testing.assert_array_equal(niter, np.array([r["niter"] for r in recs], dtype=np.int64))
    np.testing.assert_array_equal(status, np.array([r["status"] for r in recs], dtype=np.int32))
    np.testing.assert_array_equal(has, np.array([r["x_best"] is not None for r in recs], dtype=np.int32))
    assert_bits(gamma, np.array([r["gamma"] for r in recs]), "gamma")
    want = np.stack([np.full(n, np.nan) if r["x_best"] is None else r["x_best"] for r in recs])
    assert_bits(x_best, want, "x_best")   # rows without a result stay as the caller left them (NaN)


def assert_state_equal(prob, batch, recs):
    idx, val = prob.last()
    np.testing.assert_array_equal(idx, np.array([r["min_idx"] for r in recs], dtype=np.int64))
    assert_bits(val, np.array([r["min_val"] for r in recs]), "min_val")
    assert_bits(batch.mq, np.stack([r["mq"] for r in recs]), "mq")
    assert_bits(batch.xc(), np.stack([r["xc"] for r in recs]), "xc")
    assert_bits(batch.kappa, np.array([r["kappa"] for r in recs]), "kappa")
    assert_bits(batch.tsq(), np.array([r["tsq"] for r in recs]), "tsq")


def check_loop(gpu, data, lab, recs, max_iters, tol, chunk=None, batch=None):
    B, n = lab.shape[0], data.shape[-1] + 1
    prob = gpu.BatchSvmProblem(data, lab)
    if chunk is not None:
        prob.set_chunk(chunk)
    batch = new_batch(gpu, B, n) if batch is None else batch
    got = prob.optim(batch, INF, max_iters, tol)
    assert_runs_equal(got, recs, n)
    assert_state_equal(prob, batch, recs)
    return prob, batch, got


def family_arrays(members, m, nfeat):
    sets = [ref.family(s, m, nfeat) for s in members]
    return np.stack([X for X, _ in sets]), np.stack([l for _, l in sets])


def check_family(gpu, m, nfeat, tol, max_iters, members=range(16), chunk=None):
    data, lab = family_arrays(members, m, nfeat)
    recs = [ref.solve(s, m, nfeat, max_iters, tol) for s in members]
    return recs, check_loop(gpu, data, lab, recs, max_iters, tol, chunk)


@pytest.mark.parametrize("m,nfeat,tol,max_iters,niters", ref.ROWS, ids=[f"{r[0]}x{r[1]}" for r in ref.ROWS])
def test_family_per_problem_tables(gpu, m, nfeat, tol, max_iters, niters):
    """s = 0..15 in one workgroup (two at n = 16) end in every way the loop can: the zero cut, the tolerance, max_iters"""
    recs, _ = check_family(gpu, m, nfeat, tol, max_iters)
    assert tuple(r["niter"] for r in recs[:6]) == niters
    assert np.isnan(recs[0]["xc"]).all() and recs[0]["tsq"] == 0.0 and same_bits(recs[0]["gamma"], 0.0)


def test_shared_table_one_vs_rest_with_label_noise(gpu):
    m, nfeat, B, max_iters, tol = 120, 3, 16, 400, 1e-8
    rng = np.random.default_rng(11)
    cluster = np.arange(m) % 4
    centres = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0.5]])
    data = centres[cluster] + 0.4 * (rng.random((m, nfeat)) - 0.5)
    lab = np.stack([np.where(cluster == b % 4, 1, -1).astype(np.int32) for b in range(B)])
    for b in range(4, B):   # label noise: a few labels of every repeat change places
        pick = rng.choice(m, size=2 * (b // 4), replace=False)
        lab[b, pick] = lab[b, rng.permutation(pick)]
    recs = [ref.run(data, lab[b], max_iters, tol) for b in range(B)]
    assert len({r["niter"] for r in recs}) > 2
    check_loop(gpu, data, lab, recs, max_iters, tol)


@pytest.mark.parametrize("B", [1, 64, 257])
def test_copies_of_one_problem(gpu, B):
    m, nfeat, tol, max_iters, _ = ref.ROWS[0]
    recs, _ = check_family(gpu, m, nfeat, tol, max_iters, members=[1] * B)
    assert recs[0]["niter"] == 277 and recs[0]["gamma"] < 0.0


@pytest.mark.parametrize("m,nfeat,B", SHAPES)
def test_odd_shapes(gpu, m, nfeat, B):
    max_iters = 40 if nfeat == 127 else 30   # n = 128 is cut off at 40 iterations
    recs, _ = check_family(gpu, m, nfeat, 1e-10, max_iters, members=range(B))
    if nfeat == 127:
        assert max(r["niter"] for r in recs) == 40


# ---- 4. chunking ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunking_changes_nothing(gpu, chunk):
    m, nfeat, tol, max_iters, _ = ref.ROWS[0]
    check_family(gpu, m, nfeat, tol, max_iters, chunk=chunk)


# ---- 5. cut-off and resume --------------------------------------------------------------------------------------------
def test_cut_off_and_resume(gpu):
    m, nfeat, tol, _, _ = ref.ROWS[1]
    B, n, more = 16, nfeat + 1, 1500
    data, lab = family_arrays(range(B), m, nfeat)
    spaces = [ref.fresh(n) for _ in range(B)]
    first = [ref.run(data[b], lab[b], 50, tol, space=spaces[b]) for b in range(B)]
    assert {r["niter"] for r in first} > {50}   # some stopped earlier, most were cut off
    prob, batch, got = check_loop(gpu, data, lab, first, 50, tol)
    # the second call carries on: gamma and last() carry over, x_best starts empty
    second = [ref.run(data[b], lab[b], more, tol, space=spaces[b], gamma=first[b]["gamma"],
                      last=(first[b]["min_idx"], first[b]["min_val"])) for b in range(B)]
    full = ref.solve(1, m, nfeat, 3000, tol)
    assert second[1]["niter"] + 50 == full["niter"] and same_bits(second[1]["xc"], full["xc"])   # the uninterrupted run
    got2 = prob.optim(batch, got[3], more, tol)
    assert_runs_equal(got2, second, n)
    assert_state_equal(prob, batch, second)
    # max_iters = 0 moves nothing: no x_best, gamma as given, last() and the spaces as they were
    x_best, has, niter, gamma, status = prob.optim(batch, got2[3], 0, tol)
    assert not has.any() and not niter.any() and not status.any() and np.isnan(x_best).all()
    assert_bits(gamma, got2[3], "gamma")
    assert_state_equal(prob, batch, second)


def test_tol_zero_runs_past_the_zero_cut(gpu):
    m, nfeat = 64, 2
    members = [0, 3, 6]
    data, lab = family_arrays(members, m, nfeat)
    recs = [ref.run(data[b], lab[b], 10, 0.0) for b in range(3)]
    for r in recs:
        assert r["niter"] == 10 and same_bits(r["gamma"], 0.0) and np.isnan(r["xc"]).all() and np.isnan(r["tsq"])
        assert (r["min_idx"], r["min_val"]) == (0, INF)
    check_loop(gpu, data, lab, recs, 10, 0.0)


# ---- 6. interoperation ------------------------------------------------------------------------------------------------
def test_batch_update_continues_from_the_loops_spaces(gpu):
    m, nfeat, tol, _, _ = ref.ROWS[1]
    members = [1, 2, 4, 5, 7, 8, 10, 11]
    B, n = len(members), nfeat + 1
    data, lab = family_arrays(members, m, nfeat)
    spaces = [ref.fresh(n) for _ in range(B)]
    first = [ref.run(data[b], lab[b], 30, tol, space=spaces[b]) for b in range(B)]
    prob, batch, got = check_loop(gpu, data, lab, first, 30, tol)
    rng = np.random.default_rng(3)
    grads = rng.standard_normal((1, B, n))
    kinds = rng.integers(0, 2, size=(1, B)).astype(np.int32)
    beta = np.zeros((1, B))
    want = np.zeros((1, B), dtype=np.int32)
    for b, space in enumerate(spaces):
        beta[0, b] = 0.1 * np.sqrt(space.tsq) if kinds[0, b] == 0 else 0.0
        want[0, b] = space.update(int(kinds[0, b]), grads[0, b], beta[0, b])
    status, _ = batch.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    after = [dict(first[b], **ref.space_record(spaces[b])) for b in range(B)]
    assert_state_equal(prob, batch, after)
    second = [ref.run(data[b], lab[b], 200, tol, space=spaces[b], gamma=first[b]["gamma"]) for b in range(B)]
    assert_runs_equal(prob.optim(batch, got[3], 200, tol), second, n)
    assert_state_equal(prob, batch, second)


def test_from_space_output_is_valid_loop_input(gpu):
    m, nfeat, tol, max_iters, _ = ref.ROWS[0]
    B, n = 5, nfeat + 1
    data, lab = family_arrays(range(B), m, nfeat)
    recs = [ref.solve(s, m, nfeat, max_iters, tol) for s in range(B)]
    batch = gpu.EllBatch.from_space(gpu.Ell.new_with_scalar(ref.KAPPA, np.zeros(n)), B)
    check_loop(gpu, data, lab, recs, max_iters, tol, batch=batch)


def test_a_stopped_instance_beside_a_live_one_is_not_touched(gpu):
    """s = 0 stops after its third round (the zero cut); its neighbour in the same workgroup runs 277 rounds more"""
    m, nfeat, tol, max_iters, _ = ref.ROWS[0]
    recs, (prob, batch, got) = check_family(gpu, m, nfeat, tol, max_iters, members=[0, 1], chunk=16)
    assert [r["niter"] for r in recs] == [2, 277]
    alone = ref.solve(0, m, nfeat, max_iters, tol)
    assert_bits(batch.mq[0], alone["mq"], "mq")
    assert_bits(got[0][0], alone["x_best"], "x_best")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_spaces_untouched(gpu):
    lib = gpu.capi.load()
    m, nfeat, B = 64, 2, 4
    n = nfeat + 1
    data, lab = family_arrays(range(B), m, nfeat)
    prob = gpu.BatchSvmProblem(data, lab)
    rng = np.random.default_rng(2)

    def refused(batch):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        gamma = np.full(batch.B, 0.3)
        xb = np.full((batch.B, batch.n), np.nan)
        has = np.full(batch.B, -5, dtype=np.int32)
        niter = np.full(batch.B, -5, dtype=np.int64)
        status = np.full(batch.B, -5, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.ellhip_batch_svm_optim(batch._h, prob._h, ptr(gamma), 100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status))
        assert rc == gpu.capi.E_INVALID and lib.ellhip_last_error()
        for a, b in zip(before, (batch.mq, batch.xc(), batch.kappa, batch.tsq())):
            assert same_bits(a, b)
        assert np.isnan(xb).all() and (gamma == 0.3).all()
        assert (has == -5).all() and (niter == -5).all() and (status == -5).all()

    refused(gpu.EllStableBatch.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n))))
    refused(gpu.EllBatch.new_with_scalar(np.full(B + 1, 10.0), rng.standard_normal((B + 1, n))))   # wrong B
    refused(gpu.EllBatch.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n + 1))))       # wrong n
    refused(gpu.EllBatch.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, nfeat))))       # n = nfeat
    assert prob.last()[1].tolist() == [INF] * B
    with pytest.raises(gpu.capi.EllHipError):
        prob.set_chunk(0)
    with pytest.raises(gpu.capi.EllHipError):
        prob.set_chunk(4097)
    with pytest.raises(gpu.capi.EllHipError):
        gpu.BatchSvmProblem(np.zeros((2, 4, 128)), np.ones((2, 4), dtype=np.int32))
    with pytest.raises(ValueError):
        prob.assess_optim(np.zeros((B, n + 1)))
    # and the good pair still runs
    recs = [ref.solve(s, m, nfeat, 2000, 1e-12) for s in range(B)]
    batch = new_batch(gpu, B, n)
    assert_runs_equal(prob.optim(batch, INF, 2000, 1e-12), recs, n)
    assert_state_equal(prob, batch, recs)


# ---- 8. the C++ mirror ------------------------------------------------------------------------------------------------
def test_cpp_runner_matches_the_cpu_runs(gpu, tmp_path):
    import cpp_build
    m, nfeat, tol, max_iters, _ = ref.ROWS[0]
    B = 16
    data, lab = family_arrays(range(B), m, nfeat)
    path = tmp_path / "family.bin"
    path.write_bytes(struct.pack("<4qd", B, m, nfeat, max_iters, tol) + data.tobytes() + lab.astype(np.int32).tobytes())
    exe = cpp_build.build_runner("batch_svm_runner.cpp", "hip")
    got = cpp_build.run_json_lines(exe, str(path))
    assert len(got) == B
    hexbits = lambda v: format(int(np.float64(v).view(np.uint64)), "016x")
    for b in range(B):
        d, r = got[f"sweep_{b}"], ref.solve(b, m, nfeat, max_iters, tol)
        assert d["niter"] == r["niter"] and d["status"] == r["status"] and d["has_best"] == 1
        assert d["gamma"] == hexbits(r["gamma"]) and d["x_best"] == [hexbits(v) for v in r["x_best"]]
        assert d["min_idx"] == r["min_idx"] and d["min_val"] == hexbits(r["min_val"])
