"""GPU: the batched device-resident cutting-plane loops on EllStable batch handles
(include/ellhip_batch_stable_loops.h) against the CPU loops over oracle.OracleEllStable and against the host-driven form
over ellhip_batch_update (tests/batch_stable_loop_reference.py).  The row-parallel update (csrc/batch_stable_apply.hpp)
parallelises over independent outputs only, so every comparison is EXACT: np.array_equal on float64 and integers -- niter,
status, gamma, x_best / has_best, the oracle state (idx; the low-pass cursors, kmax, fmax, sp_sq; the SVM min_idx / min_val)
and the spaces: mq with its scratch triangle, xc, kappa and tsq.  NaN is compared as a pattern where the reference itself
produces it (n = 1 after one cut; the SVM's zero cut)."""
import ctypes as C
import math

import numpy as np
import pytest

import batch_lmi_reference as lmi
import batch_lowpass_reference as lp
import batch_stable_loop_reference as ref

pytestmark = pytest.mark.gpu


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    nan = a.dtype.kind == "f"
    assert np.array_equal(a, b, equal_nan=nan), f"{what}: {np.argwhere(~((a == b) | ((a != a) & (b != b))))[:4].tolist()}"


def make_gpu(gpu, case, chunk=None):
    if case.kind.startswith("lmi"):
        mat_f, mat_b, c = lmi.stack(case.problems)
        prob = gpu.BatchLmiProblem(mat_f, mat_b, c if case.kind == "lmi_optim" else None)
    elif case.kind.startswith("lp"):
        prob = gpu.BatchLowpassProblem(case.n, *lp.columns(case.problems))
    elif case.shared:
        prob = gpu.BatchSvmProblem(case.problems[0][0], np.stack([p[1] for p in case.problems]))
    else:
        prob = gpu.BatchSvmProblem(np.stack([p[0] for p in case.problems]), np.stack([p[1] for p in case.problems]))
    if chunk is not None:
        prob.set_chunk(chunk)
    return prob, make_batch(gpu, case)


def make_batch(gpu, case):
    if case.mq is None:
        batch = gpu.EllStableBatch.new_with_scalar(case.kappa, case.xc)
    else:
        batch = gpu.EllStableBatch.new_with_matrix(case.kappa, case.mq, case.xc)
    assert batch.variant == gpu.capi.SPACE_ELL_STABLE
    if not case.use_parallel:
        batch.set_use_parallel_cut(False)
    return batch


def run_device(prob, batch, case, gamma=None, max_iters=None):
    """-> records shaped like the reference's"""
    max_iters = case.max_iters if max_iters is None else max_iters
    if case.optim:
        x, has, niter, gamma, status = prob.optim(batch, case.gamma if gamma is None else gamma, max_iters, case.tol)
    else:
        x, has, niter, status = prob.feas(batch, max_iters, case.tol)
        gamma = case.gamma
    mq, xc, kappa, tsq = batch.mq, batch.xc(), batch.kappa, batch.tsq()
    if case.kind.startswith("lmi"):
        states = [dict(idx=int(i)) for i in prob.idx]
    elif case.kind.startswith("lp"):
        st = prob.state()
        states = [{k: st[k][b] for k in lp.STATE_KEYS} for b in range(case.B)]
    else:
        idx, val = prob.last()
        states = [dict(min_idx=int(i), min_val=v) for i, v in zip(idx, val)]
    return [dict(x_best=x[b] if has[b] else None, niter=int(niter[b]), gamma=gamma[b], status=int(status[b]),
                 state=states[b], mq=mq[b], xc=xc[b], kappa=kappa[b], tsq=tsq[b]) for b in range(case.B)]


def assert_records_equal(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        tag = f"{what} instance {b}"
        assert g["niter"] == w["niter"] and g["status"] == w["status"], (tag, g["niter"], w["niter"], g["status"], w["status"])
        same(g["gamma"], w["gamma"], tag + " gamma")
        assert (g["x_best"] is None) == (w["x_best"] is None), tag + " has_best"
        if w["x_best"] is not None:
            same(g["x_best"], w["x_best"], tag + " x_best")
        assert g["state"].keys() == w["state"].keys()
        for k in w["state"]:
            same(g["state"][k], w["state"][k], f"{tag} {k}")
        for k in ("mq", "xc", "kappa", "tsq"):
            same(g[k], w[k], f"{tag} {k}")


def check(gpu, case, chunk=None):
    """the device loop against the CPU loop and against the host-driven form; -> the CPU records"""
    want = ref.cpu_run(case)
    prob, batch = make_gpu(gpu, case, chunk)
    got = run_device(prob, batch, case)
    assert_records_equal(got, want, "device loop vs CPU")
    hosted = ref.host_driven(make_batch(gpu, case), case)
    assert_records_equal(got, hosted, "device loop vs host-driven")
    return want


# ---- LMI ----------------------------------------------------------------------------------------------------------------
def test_lmi_family_a(gpu):
    # 67 instances of n = 3: 64 per workgroup, a ragged second workgroup
    want = check(gpu, ref.lmi_case([lmi.family_a(s) for s in range(67)]))
    assert all(w["status"] == ref.NOSOLN and w["x_best"] is not None and 15 <= w["niter"] <= 40 for w in want[:4])
    assert len({w["niter"] for w in want}) > 1  # instances of one workgroup stop at different iterations


def test_lmi_family_b_n5(gpu):
    want = check(gpu, ref.lmi_case([lmi.family_b(s, 5, 6, 2) for s in range(6)]))
    assert max(w["niter"] for w in want) > 200 and all(w["niter"] < 2000 for w in want)


def test_lmi_family_b_n16_capped(gpu):
    want = check(gpu, ref.lmi_case([lmi.family_b(s, 16, 12, 3) for s in range(5)], max_iters=300))
    assert all(w["niter"] == 300 and w["status"] == ref.SUCCESS for w in want)


@pytest.mark.parametrize("family", ["A", "B"])
def test_lmi_feas(gpu, family):
    problems = [lmi.family_a(s) if family == "A" else lmi.family_b(s, 5, 6, 2) for s in range(8)]
    case = ref.lmi_feas_case(problems)
    want = check(gpu, case)
    # a case in which no instance runs an update shows nothing
    assert sum(w["niter"] >= 2 for w in want) >= 4
    assert any(w["x_best"] is not None for w in want)
    for b, w in enumerate(want):  # an instance that is feasible where it starts is never touched
        if w["niter"] == 0 and w["x_best"] is not None:
            same(w["xc"], case.xc[b], "untouched xc")
            same(w["mq"], np.eye(case.n), "untouched mq")


# ---- low-pass -----------------------------------------------------------------------------------------------------------
def test_lowpass_loose_and_family_n8(gpu):
    # LOOSE runs ~1350 iterations while the family members of the same workgroup stop after 11..94
    consts = [lp.LOOSE] + [lp.family(s) for s in range(6)]
    want = check(gpu, ref.lp_case(8, consts))
    assert want[0]["niter"] > 1000 and want[0]["x_best"] is not None
    assert all(w["status"] == ref.NOSOLN for w in want[1:]) and len({w["niter"] for w in want[1:]}) > 1
    want = check(gpu, ref.lp_case(8, consts, feas=True))
    assert want[0]["x_best"] is not None and want[0]["niter"] > 20


@pytest.mark.parametrize("n", [16, 32])
def test_lowpass_family(gpu, n):
    consts = [lp.family(s) for s in range(6)] + [lp.FEAS_INFEASIBLE, lp.NO_STOPBAND_A]
    check(gpu, ref.lp_case(n, consts, max_iters=400))
    want = check(gpu, ref.lp_case(n, consts, feas=True, max_iters=400))
    if n == 16:
        assert want[6]["x_best"] is None and want[6]["status"] == ref.NOSOLN
        assert want[7]["x_best"] is not None


def test_lowpass_no_stopband_ends_unknown(gpu):
    want = check(gpu, ref.lp_case(16, [lp.NO_STOPBAND_A, lp.LOOSE], max_iters=400))
    assert want[0]["status"] == ref.UNKNOWN and want[0]["niter"] > 100


def test_lowpass_short_passband_n32(gpu):
    want = check(gpu, ref.lp_case(32, [lp.SHORT_PASSBAND, lp.family(1)], feas=True))
    assert want[0]["x_best"] is not None and want[0]["niter"] > 100
    want = check(gpu, ref.lp_case(32, [lp.SHORT_PASSBAND, lp.family(1)], max_iters=300))
    assert want[0]["niter"] == 300


def test_lowpass_without_parallel_cuts(gpu):
    consts = [lp.LOOSE] + [lp.family(s) for s in range(4)]
    with_pc = ref.cpu_run(ref.lp_case(8, consts, max_iters=400))
    want = check(gpu, ref.lp_case(8, consts, max_iters=400, use_parallel=False))
    assert any(a["niter"] != b["niter"] or not np.array_equal(a["xc"], b["xc"]) for a, b in zip(with_pc, want))


# ---- SVM ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("m,nfeat,tol", [(64, 2, 1e-12), (96, 7, 1e-8)])
def test_svm(gpu, m, nfeat, tol, shared):
    want = check(gpu, ref.svm_case(m, nfeat, tol, range(6), shared=shared))
    if not shared:
        assert max(w["niter"] for w in want) > 200
        assert min(w["niter"] for w in want) < 10  # the separable members end on the zero cut


# ---- shapes where the row-parallel update can go wrong -------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_smallest_dimensions(gpu, n):
    """n = 1: no forward step, last_idx = 0; the reference's state goes NaN after one cut, the NaN pattern is compared"""
    problems = [lmi.family_b(s, n, 3, 2) for s in range(70)]
    want = check(gpu, ref.lmi_case(problems, max_iters=60))
    assert any(w["niter"] >= 1 for w in want)
    check(gpu, ref.lmi_case(problems, max_iters=60).with_random_factors(n))


@pytest.mark.parametrize("n", [63, 64, 65])
def test_an_instance_crosses_a_wave(gpu, n):
    want = check(gpu, ref.lmi_case([lmi.family_b(s, n, 4, 2) for s in range(5)], max_iters=40).with_random_factors(n))
    assert max(w["niter"] for w in want) >= 10


def test_largest_dimension(gpu):
    """n = 128, the largest buffer each oracle admits under the LDS bound"""
    want = check(gpu, ref.lmi_case([lmi.family_b(s, 128, 8, 2) for s in range(2)], max_iters=20).with_random_factors(128))
    assert max(w["niter"] for w in want) >= 10
    check(gpu, ref.lp_case(128, [lp.LOOSE, lp.family(2)], max_iters=20))
    check(gpu, ref.svm_case(64, 127, 1e-8, range(1, 3), max_iters=20))


# ---- start states -------------------------------------------------------------------------------------------------------
def test_random_factor_start_states(gpu):
    check(gpu, ref.lmi_case([lmi.family_b(s, 5, 6, 2) for s in range(6)], max_iters=400).with_random_factors(1))
    check(gpu, ref.lp_case(16, [lp.family(s) for s in range(6)]).with_random_factors(2))
    check(gpu, ref.svm_case(64, 2, 1e-12, range(6), max_iters=400).with_random_factors(3))


def test_spaces_from_one_handle(gpu):
    case = ref.lmi_case([lmi.family_a(s) for s in range(9)])
    want = ref.cpu_run(case)
    prob, _ = make_gpu(gpu, case)
    batch = gpu.EllStableBatch.from_space(gpu.EllStable.new_with_scalar(10.0, np.zeros(3)), case.B)
    assert_records_equal(run_device(prob, batch, case), want, "from_space")


# ---- loop mechanics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunking_changes_nothing(gpu, chunk):
    for case in (ref.lmi_case([lmi.family_a(s) for s in range(67)]),
                 ref.lp_case(8, [lp.family(s) for s in range(6)]),
                 ref.svm_case(64, 2, 1e-12, range(6), max_iters=100)):
        want = ref.cpu_run(case)
        prob, batch = make_gpu(gpu, case, chunk)
        assert_records_equal(run_device(prob, batch, case), want, f"chunk {chunk} {case.kind}")


def test_cut_off_and_resume_equals_one_long_run(gpu):
    for case, cut in ((ref.lmi_case([lmi.family_b(s, 5, 6, 2) for s in range(6)]), 50),
                      (ref.lp_case(8, [lp.LOOSE] + [lp.family(s) for s in range(3)]), 40),
                      (ref.svm_case(64, 2, 1e-12, range(6)), 30)):
        long_run = ref.cpu_run(case)
        assert any(w["niter"] > cut for w in long_run)
        prob, batch = make_gpu(gpu, case)
        first = run_device(prob, batch, case, max_iters=cut)
        assert all(f["niter"] == min(cut, w["niter"]) for f, w in zip(first, long_run))
        # the instances that were cut off go on (the others, which had ended, are not looked at again)
        going = [b for b, w in enumerate(long_run) if w["niter"] > cut]
        second = run_device(prob, batch, case, gamma=np.array([f["gamma"] for f in first]), max_iters=case.max_iters)
        for b in going:
            s, w = second[b], long_run[b]
            assert first[b]["status"] == ref.SUCCESS
            assert cut + s["niter"] == w["niter"] and s["status"] == w["status"], (case.kind, b)
            same(s["gamma"], w["gamma"], "gamma")
            for k in ("mq", "xc", "kappa", "tsq"):
                same(s[k], w[k], f"{case.kind} resumed {b} {k}")
            for k in w["state"]:
                same(s["state"][k], w["state"][k], f"{case.kind} resumed {b} {k}")
            if s["x_best"] is not None:  # a best point of the second call is the long run's
                same(s["x_best"], w["x_best"], "x_best")


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(gpu):
    lib = gpu.capi.load()
    rng = np.random.default_rng(2)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lmi_case = ref.lmi_case([lmi.family_a(s) for s in range(4)])
    mat_f, mat_b, c = lmi.stack(lmi_case.problems)
    probs = {
        "ellhip_batch_lmi_optim_stable": (gpu.BatchLmiProblem(mat_f, mat_b, c), 3, True),
        "ellhip_batch_lmi_feas_stable": (gpu.BatchLmiProblem(mat_f, mat_b, None), 3, False),
        "ellhip_batch_lowpass_optim_stable": (gpu.BatchLowpassProblem(8, *lp.columns([lp.LOOSE] * 4)), 8, True),
        "ellhip_batch_lowpass_feas_stable": (gpu.BatchLowpassProblem(8, *lp.columns([lp.LOOSE] * 4)), 8, False),
        "ellhip_batch_svm_optim_stable": (gpu.BatchSvmProblem(rng.random((4, 64, 2)), np.ones((4, 64), dtype=np.int32)), 3,
                                          True),
    }
    assert sorted(probs) == sorted(gpu.capi.BATCH_STABLE_LOOP_EXPORTS)

    def refused(entry, batch, prob, optim):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        gamma = np.full(batch.B, 0.3)
        xb = np.full((batch.B, batch.n), np.nan)
        has = np.full(batch.B, -5, dtype=np.int32)
        niter = np.full(batch.B, -5, dtype=np.int64)
        status = np.full(batch.B, -5, dtype=np.int32)
        args = ([ptr(gamma)] if optim else []) + [100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status)]
        assert getattr(lib, entry)(batch._h, prob._h, *args) == gpu.capi.E_INVALID and lib.ellhip_last_error()
        for a, b in zip(before, (batch.mq, batch.xc(), batch.kappa, batch.tsq())):
            same(a, b, entry + " space")
        assert np.isnan(xb).all() and (gamma == 0.3).all()
        assert (has == -5).all() and (niter == -5).all() and (status == -5).all()

    for entry, (prob, n, optim) in probs.items():
        stable = lambda B, nn: gpu.EllStableBatch.new_with_matrix(
            np.full(B, 10.0), np.stack([ref.random_factor(nn, 7 + b) for b in range(B)]), rng.standard_normal((B, nn)))
        refused(entry, gpu.EllBatch.new_with_scalar(np.full(4, 10.0), rng.standard_normal((4, n))), prob, optim)  # an Ell handle
        refused(entry, stable(5, n), prob, optim)      # wrong B
        refused(entry, stable(4, n + 1), prob, optim)  # wrong n
    # one shape just beyond the LDS bound: n = 128 with a 64 x 64 block (n = 128 with 8 x 8 blocks runs, see above)
    big = gpu.BatchLmiProblem([np.zeros((1, 128, 64, 64))], [np.eye(64)[None]], np.ones((1, 128)))
    refused("ellhip_batch_lmi_optim_stable", gpu.EllStableBatch.new_with_scalar(np.full(1, 10.0), np.zeros((1, 128))), big,
            True)
    # and the Python mirror picks the entry point by the handle's variant
    with pytest.raises(gpu.capi.EllHipError, match="differ in B or n"):
        probs["ellhip_batch_svm_optim_stable"][0].optim(
            gpu.EllStableBatch.new_with_scalar(np.full(5, 10.0), np.zeros((5, 3))), math.inf, 10, 1e-8)
