"""GPU: the streamed batch engine (include/ellhip_batch_streamed.h) against the CPU oracle and against the LDS engine,
through the C ABI.  The engine follows the reference's statement order, so every comparison is on bit patterns (NaNs
compared by position: the payload of a NaN is not part of the reference's contract)."""
import ctypes as C

import numpy as np
import pytest

from util import mixed_cut, oracle_update, rel_inf

pytestmark = pytest.mark.gpu


def same_bits(a, b, what=""):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na = np.isnan(a)
    np.testing.assert_array_equal(na, np.isnan(b), err_msg=what + ": NaN positions")
    np.testing.assert_array_equal(a[~na].view(np.uint64), b[~na].view(np.uint64), err_msg=what + ": bits")


def assert_state(batch, ors, what=""):
    same_bits(batch.mq, np.stack([o.mq for o in ors]), what + " mq")
    same_bits(batch.xc(), np.stack([np.array(o.xc) for o in ors]), what + " xc")
    same_bits(batch.kappa, np.array([o.kappa for o in ors]), what + " kappa")
    same_bits(batch.tsq(), np.array([o.tsq for o in ors]), what + " tsq")


def apply_cuts(batch, ors, kinds, grads, b0, b1):
    """One launch of K cuts on the batch, the same cuts one by one on the oracles; every status and tsq compared.
    kinds, b0, b1: [K][B] (b1 NaN = no second value), grads [K][B][n].  Returns the statuses."""
    K, B = kinds.shape
    want = np.zeros((K, B), dtype=np.int32)
    want_tsq = np.zeros((K, B))
    for k in range(K):
        for b, o in enumerate(ors):
            want[k, b] = oracle_update(o, int(kinds[k, b]), grads[k, b], float(b0[k, b]),
                                       None if np.isnan(b1[k, b]) else float(b1[k, b]))
            want_tsq[k, b] = o.tsq
    status, tsq = batch.update(kinds, grads, b0, b1)
    np.testing.assert_array_equal(status, want)
    same_bits(tsq, want_tsq, "tsq per cut")
    return status


def make(gpu, orc, B, n, rng, *, nonsym=False):
    kappa = 0.5 + 2.0 * rng.random(B)
    xc0 = rng.standard_normal((B, n))
    if nonsym:
        mq = np.stack([np.eye(n) * (1.0 + rng.random()) + (0.1 / n) * rng.standard_normal((n, n)) for _ in range(B)])
        batch = gpu.EllBatchStreamed.new_with_matrix(kappa, mq, xc0)
        ors = [orc.OracleEll.new_with_matrix(kappa[b], mq[b], xc0[b]) for b in range(B)]
        return batch, ors, mq
    batch = gpu.EllBatchStreamed.new_with_scalar(kappa, xc0)
    ors = [orc.OracleEll.new_with_scalar(kappa[b], xc0[b]) for b in range(B)]
    return batch, ors, None


def mixed_round(ors, K, n, rng, it):
    """K mixed cuts per ellipsoid (tests/util.py: mixed_cut), beta scaled by each oracle's tau at the START of the round:
    the oracles are not advanced here, apply_cuts does that."""
    B = len(ors)
    kinds = np.zeros((K, B), dtype=np.int32)
    grads = rng.standard_normal((K, B, n))
    b0 = np.zeros((K, B))
    b1 = np.full((K, B), np.nan)
    for b, o in enumerate(ors):
        q = o.mq
        for k in range(K):
            g = grads[k, b]
            tau = np.sqrt(max(o.kappa * float(g @ (q @ g)), 0.0))
            kind, c0, c1 = mixed_cut(it + k + b, g, tau, rng)
            kinds[k, b], b0[k, b] = kind, c0
            if c1 is not None:
                b1[k, b] = c1
    return kinds, grads, b0, b1


def drive(gpu, orc, B, n, K, rounds, seed, *, no_defer=False, nonsym=False, use_parallel=True):
    rng = np.random.default_rng(seed)
    batch, ors, _ = make(gpu, orc, B, n, rng, nonsym=nonsym)
    assert batch.is_streamed and batch.variant == gpu.capi.SPACE_ELL and (batch.B, batch.n) == (B, n)
    if no_defer:
        batch.set_no_defer_trick(True)
        for o in ors:
            o.set_no_defer_trick(True)
    if not use_parallel:
        batch.set_use_parallel_cut(False)
        for o in ors:
            o.set_use_parallel_cut(False)
    counts = np.zeros(4, dtype=int)
    for r in range(rounds):
        status = apply_cuts(batch, ors, *mixed_round(ors, K, n, rng, r * K))
        counts += np.bincount(status.ravel(), minlength=4)
    assert_state(batch, ors)
    return counts


# ---- 1. exact against the CPU oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 130, 191, 192, 193, 255, 256, 257, 383, 511, 512, 513, 1000, 1023, 1024])
def test_streamed_bit_identical_to_oracle(gpu, orc, n):
    counts = drive(gpu, orc, 3, n, K=3, rounds=2, seed=2000 + n)
    assert counts[0] > 0


# ---- 2. exact against the LDS engine -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 63, 64, 65, 128])
def test_streamed_equals_the_lds_engine(gpu, orc, n):
    B, K = 37, 4
    rng = np.random.default_rng(300 + n)
    kappa = 0.5 + 2.0 * rng.random(B)
    xc0 = rng.standard_normal((B, n))
    lds = gpu.EllBatch.new_with_scalar(kappa, xc0)
    st = gpu.EllBatchStreamed.new_with_scalar(kappa, xc0)
    ors = [orc.OracleEll.new_with_scalar(kappa[b], xc0[b]) for b in range(B)] if n == 1 else None
    assert st.is_streamed
    seen = np.zeros(4, dtype=int)
    for r in range(3):
        q, kap = lds.mq, lds.kappa
        kinds = np.zeros((K, B), dtype=np.int32)
        grads = rng.standard_normal((K, B, n))
        b0 = np.zeros((K, B))
        b1 = np.full((K, B), np.nan)
        for k in range(K):
            with np.errstate(invalid="ignore"):  # n = 1: kappa turns inf and the matrix 0 (cst1 = inf)
                tau = np.sqrt(np.maximum(kap * np.einsum("bi,bij,bj->b", grads[k], q, grads[k]), 0.0))
            for b in range(B):
                kind, c0, c1 = mixed_cut(r * K + k + b, grads[k, b], tau[b], rng)
                kinds[k, b], b0[k, b] = kind, c0
                if c1 is not None:
                    b1[k, b] = c1
        if ors is not None:
            status_s = apply_cuts(st, ors, kinds, grads, b0, b1)
            tsq_s = None
        else:
            status_s, tsq_s = st.update(kinds, grads, b0, b1)
        status_l, tsq_l = lds.update(kinds, grads, b0, b1)
        np.testing.assert_array_equal(status_s, status_l)
        if tsq_s is not None:
            same_bits(tsq_s, tsq_l, "tsq per cut")
        seen += np.bincount(status_l.ravel(), minlength=4)
        same_bits(st.mq, lds.mq, "mq")
        same_bits(st.xc(), lds.xc(), "xc")
        same_bits(st.kappa, lds.kappa, "kappa")
        same_bits(st.tsq(), lds.tsq(), "tsq")
    if ors is not None:
        assert_state(st, ors)
    else:
        assert seen[0] > 0 and seen[1:].sum() > 0


# ---- 3. directed launches: a failure inside a fused launch is followed correctly -----------------------------------------
def directed(gpu, orc, n, seed):
    rng = np.random.default_rng(seed)
    B = 2
    batch, ors, _ = make(gpu, orc, B, n, rng)
    return rng, B, batch, ors


def cuts(rng, B, n, spec):
    """spec: one (kind, beta0, beta1) per cut of the launch, the same for every ellipsoid; fresh normal gradients"""
    K = len(spec)
    kinds = np.array([[s[0]] * B for s in spec], dtype=np.int32)
    b0 = np.array([[s[1]] * B for s in spec], dtype=np.float64)
    b1 = np.array([[s[2]] * B for s in spec], dtype=np.float64)
    return kinds, rng.standard_normal((K, B, n)), b0, b1


OK_CUT = (0, 0.01, np.nan)
NOSOLN = (0, np.inf, np.nan)


@pytest.mark.parametrize("n", [130, 257])
def test_first_cut_fails_then_successes(gpu, orc, n):
    rng, B, batch, ors = directed(gpu, orc, n, 40 + n)
    status = apply_cuts(batch, ors, *cuts(rng, B, n, [NOSOLN, OK_CUT, (1, 0.0, np.nan), OK_CUT]))
    assert status[:, 0].tolist() == [1, 0, 0, 0]
    assert_state(batch, ors)


@pytest.mark.parametrize("n", [130, 257])
def test_failures_between_successes(gpu, orc, n):
    rng, B, batch, ors = directed(gpu, orc, n, 50 + n)
    # a q-cut far on the other side of the centre (tau + n * beta < 0) answers NoEffect (EllCalc::calc_bias_cut_q)
    spec = [OK_CUT, NOSOLN, OK_CUT, (2, -1e3, np.nan), OK_CUT]
    status = apply_cuts(batch, ors, *cuts(rng, B, n, spec))
    assert status[:, 0].tolist() == [0, 1, 0, 2, 0]
    assert_state(batch, ors)


@pytest.mark.parametrize("n", [130, 257])
def test_last_cut_fails(gpu, orc, n):
    rng, B, batch, ors = directed(gpu, orc, n, 60 + n)
    status = apply_cuts(batch, ors, *cuts(rng, B, n, [OK_CUT, OK_CUT, NOSOLN]))
    assert status[:, 0].tolist() == [0, 0, 1]
    assert_state(batch, ors)
    status = apply_cuts(batch, ors, *cuts(rng, B, n, [OK_CUT]))   # and the launch after it starts from the right state
    assert status[:, 0].tolist() == [0]
    assert_state(batch, ors)


@pytest.mark.parametrize("n", [130, 257])
def test_one_cut_five_times_equals_five_cuts_once(gpu, orc, n):
    rng = np.random.default_rng(70 + n)
    B = 3
    kappa = 0.5 + 2.0 * rng.random(B)
    xc0 = rng.standard_normal((B, n))
    one = gpu.EllBatchStreamed.new_with_scalar(kappa, xc0)
    five = gpu.EllBatchStreamed.new_with_scalar(kappa, xc0)
    kinds, grads, b0, b1 = cuts(rng, B, n, [OK_CUT, (1, 0.0, 0.3), OK_CUT, (2, 0.005, np.nan), (0, 0.02, np.nan)])
    st5, ts5 = five.update(kinds, grads, b0, b1)
    for k in range(5):
        st1, ts1 = one.update(kinds[k], grads[k], b0[k], b1[k:k + 1])
        np.testing.assert_array_equal(st1[0], st5[k])
        same_bits(ts1[0], ts5[k], "tsq")
    assert np.all(st5 == 0)
    same_bits(one.mq, five.mq, "mq")
    same_bits(one.xc(), five.xc(), "xc")
    same_bits(one.kappa, five.kappa, "kappa")
    same_bits(one.tsq(), five.tsq(), "tsq")


@pytest.mark.parametrize("n", [130, 257])
def test_zero_gradient_then_an_ordinary_cut(gpu, orc, n):
    """omega = 0: the reference divides by it and its state turns NaN; the cut after it works on that state"""
    rng, B, batch, ors = directed(gpu, orc, n, 80 + n)
    kinds, grads, b0, b1 = cuts(rng, B, n, [(1, 0.0, np.nan), OK_CUT, OK_CUT])
    grads[0] = 0.0
    apply_cuts(batch, ors, kinds, grads, b0, b1)
    assert np.isnan(batch.mq).any()
    assert_state(batch, ors)


# ---- 4. flags ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [130, 256, 1024])
def test_no_defer_trick_and_use_parallel_cut(gpu, orc, n):
    drive(gpu, orc, 3, n, K=4, rounds=2, seed=7 + n, no_defer=True)
    drive(gpu, orc, 3, n, K=2, rounds=2, seed=8 + n, use_parallel=False)


# ---- 5. a matrix that is not symmetric ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 200, 513])
def test_non_symmetric_input_is_kept_until_the_first_success_mirrors_it(gpu, orc, n):
    rng = np.random.default_rng(90 + n)
    B = 3
    batch, ors, mq = make(gpu, orc, B, n, rng, nonsym=True)
    same_bits(batch.mq, mq, "mq as given")
    status = apply_cuts(batch, ors, *cuts(rng, B, n, [NOSOLN]))
    assert np.all(status == 1)
    same_bits(batch.mq, mq, "mq after a launch whose only cut failed")
    assert not np.array_equal(batch.mq[0], batch.mq[0].T)
    for r in range(2):   # the first launch mirrors (its first success on the true rows, the rest fused), the second is symmetric
        status = apply_cuts(batch, ors, *mixed_round(ors, 3, n, rng, 3 * r))
    assert (status == 0).any()
    assert_state(batch, ors)
    q = batch.mq
    same_bits(q, np.swapaxes(q, 1, 2), "mirrored")


def test_non_symmetric_input_failure_then_success_in_one_launch(gpu, orc):
    n, B = 200, 2
    rng = np.random.default_rng(17)
    batch, ors, _ = make(gpu, orc, B, n, rng, nonsym=True)
    status = apply_cuts(batch, ors, *cuts(rng, B, n, [NOSOLN, OK_CUT, OK_CUT, NOSOLN, OK_CUT]))
    assert status[:, 0].tolist() == [1, 0, 0, 1, 0]
    assert_state(batch, ors)


# ---- 6. the remaining entry points ------------------------------------------------------------------------------------------
def test_diag_constructor_set_xc_and_one_cut_per_call(gpu, orc):
    B, n = 5, 150
    rng = np.random.default_rng(3)
    diag = 0.5 + rng.random((B, n))
    xc0 = rng.standard_normal((B, n))
    batch = gpu.EllBatchStreamed.new(diag, xc0)
    ors = [orc.OracleEll.new(diag[b], xc0[b]) for b in range(B)]
    assert_state(batch, ors, "as constructed")
    for _ in range(3):
        g = rng.standard_normal((B, n))
        status, _ = batch.update(np.zeros(B, dtype=np.int32), g, np.full(B, 0.01))
        for b in range(B):
            assert status[0, b] == ors[b].update_bias_cut(g[b], 0.01) == 0
        assert_state(batch, ors)
    x = rng.standard_normal((B, n))
    batch.set_xc(x)
    for b, o in enumerate(ors):
        o.set_xc(x[b])
    same_bits(batch.xc(), x, "set_xc")
    apply_cuts(batch, ors, *cuts(rng, B, n, [OK_CUT]))
    assert_state(batch, ors)


def _hip(gpu):
    """The HIP runtime the engine is bound to (the package may have opened PyTorch-ROCm's copy, capi.load)."""
    paths = sorted(gpu.capi.mapped_runtimes()["libamdhip64"])
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_update_dev_gives_the_bits_of_update(gpu):
    """The same cuts through ellhip_batch_update_dev (arrays already in HBM) and ellhip_batch_update."""
    n, B, K = 257, 5, 5
    rng = np.random.default_rng(31)
    xc0 = rng.standard_normal((B, n))
    a = gpu.EllBatchStreamed.new_with_scalar(2.0, xc0)
    d = gpu.EllBatchStreamed.new_with_scalar(2.0, xc0)
    kinds = rng.integers(0, 3, (K, B)).astype(np.int32)
    grads = rng.standard_normal((K, B, n))
    b0 = 0.01 * rng.random((K, B))
    has1 = (rng.random((K, B)) < 0.5).astype(np.int32)
    b1 = np.where(has1 == 1, 0.5 + rng.random((K, B)), 0.0)
    st_a, ts_a = a.update(kinds, grads, b0, np.where(has1 == 1, b1, np.nan))
    hip = _hip(gpu)
    host = [np.ascontiguousarray(x) for x in (kinds, grads, b0, has1, b1)]
    outs = [np.zeros((K, B), dtype=np.int32), np.zeros((K, B))]
    ptrs = []
    try:
        for x in host + outs:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), x.nbytes) == 0
            ptrs.append(p)
        for p, x in zip(ptrs, host):
            assert hip.hipMemcpy(p, x.ctypes.data, x.nbytes, 1) == 0
        d.update_dev(K, *ptrs)
        d.synchronize()
        for p, x in zip(ptrs[len(host):], outs):
            assert hip.hipMemcpy(x.ctypes.data, p, x.nbytes, 2) == 0
    finally:
        for p in ptrs:
            hip.hipFree(p)
    np.testing.assert_array_equal(outs[0], st_a)
    same_bits(outs[1], ts_a, "tsq per cut")
    assert (st_a == 0).any()
    for get in ("mq", "kappa"):
        same_bits(getattr(d, get), getattr(a, get), get)
    same_bits(d.xc(), a.xc(), "xc")
    same_bits(d.tsq(), a.tsq(), "tsq")


# ---- 7. from_space --------------------------------------------------------------------------------------------------------
def test_from_space_clones_an_ell(gpu, orc):
    """BSearchAdaptor pattern (src/cutting_plane.rs:410): B probes start from clones of one space.  The clone is the
    single handle's matrix to the bit; that handle itself follows the oracle within the suite's relative inf-norm
    (tests/util.py: rel_inf), not element by element: its products are summed in another order, so an off-diagonal
    element of 1e-5 carries the absolute error of the elements of 1 next to it.  The bounds are those of the LDS engine's
    from_space test, in that norm."""
    n, B = 300, 6
    rng = np.random.default_rng(5)
    x0 = rng.standard_normal(n)
    for depth in (1, 8):
        base = gpu.Ell.new_with_scalar(3.0, x0)
        base.defer_depth = depth
        obase = orc.OracleEll.new_with_scalar(3.0, x0)
        for _ in range(3):  # at depth 8 these stay recorded until the clone forces them into Q
            g = rng.standard_normal(n)
            assert int(base.update_bias_cut((g, 0.05))) == obase.update_bias_cut(g, 0.05) == 0
        batch = gpu.EllBatchStreamed.from_space(base, B)
        assert batch.is_streamed and (batch.B, batch.n) == (B, n)
        mq = batch.mq
        if depth == 1:
            same_bits(mq[0], base.mq, "clone")
        print(f"from_space n={n} depth={depth}: clone vs oracle rel_inf {rel_inf(mq[B - 1], obase.mq):.3e}")
        assert rel_inf(mq[B - 1], obase.mq) <= 1e-12
        assert np.array_equal(batch.xc()[2], base.xc()) and batch.kappa[3] == base.kappa
        # probes diverge from here: different cuts per clone, each equal to a clone of the single space
        probes = [base.clone() for _ in range(B)]
        g = rng.standard_normal((B, n))
        beta = 0.01 * (1 + np.arange(B))
        status, _ = batch.update(np.zeros(B, dtype=np.int32), g, beta)
        mq, xc = batch.mq, batch.xc()
        for b in range(B):
            assert status[0, b] == int(probes[b].update_bias_cut((g[b], float(beta[b]))))
            eq, ex = rel_inf(mq[b], probes[b].mq), rel_inf(xc[b], probes[b].xc())
            print(f"from_space n={n} depth={depth} probe {b}: rel_inf mq {eq:.3e} xc {ex:.3e}")
            assert eq <= 1e-11 and ex <= 1e-11


# ---- 8. more workgroups than the card holds at once ------------------------------------------------------------------------
def test_large_population(gpu, orc):
    B, n, K = 4000, 129, 2
    rng = np.random.default_rng(11)
    batch = gpu.EllBatchStreamed.new_with_scalar(1.0, np.zeros((B, n)))
    grads = rng.standard_normal((K, B, n))
    beta = 0.05 * rng.random((K, B))
    status, tsq = batch.update(np.zeros((K, B), dtype=np.int32), grads, beta)
    assert np.all(status == 0)
    mq, xc, kap = batch.mq, batch.xc(), batch.kappa
    for b in rng.choice(B, 12, replace=False):
        o = orc.OracleEll.new_with_scalar(1.0, np.zeros(n))
        for k in range(K):
            assert o.update_bias_cut(grads[k, b], beta[k, b]) == 0
            same_bits(tsq[k, b], o.tsq, "tsq")
        same_bits(mq[b], o.mq, "mq")
        same_bits(xc[b], np.array(o.xc), "xc")
        same_bits(kap[b], o.kappa, "kappa")


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    capi = gpu.capi
    lib = capi.load()
    h = C.c_void_p()
    assert lib.ellhip_batch_create_streamed(C.byref(h), 2, 1025, None, None, None, None, -1) == capi.E_INVALID and not h.value
    assert lib.ellhip_batch_create_streamed(C.byref(h), 0, 16, None, None, None, None, -1) == capi.E_INVALID and not h.value
    with pytest.raises(capi.EllHipError):
        gpu.EllBatchStreamed.new_with_scalar(np.ones(2), np.zeros((2, 1025)))
    with pytest.raises(capi.EllHipError):
        gpu.EllBatch.new_with_scalar(np.ones(2), np.zeros((2, 129)))   # the LDS engine keeps its limit
    with pytest.raises(capi.EllHipError):
        gpu.EllBatchStreamed.from_space(gpu.EllStable.new_with_scalar(1.0, np.zeros(4)), 3)
    assert lib.ellhip_batch_is_streamed(gpu.EllBatch.new_with_scalar(1.0, np.zeros((2, 4)))._h) == 0
    assert lib.ellhip_batch_is_streamed(None) == capi.E_INVALID


def test_batched_loops_refuse_a_streamed_handle(gpu):
    """also at n <= 128, where the shapes would match: those kernels assume the LDS layout"""
    capi = gpu.capi
    lib = capi.load()
    n, B = 16, 2
    rng = np.random.default_rng(2)
    batch = gpu.EllBatchStreamed.new_with_scalar(40.0, np.zeros((B, n)))
    before = batch.mq
    x = np.zeros((B, n))
    i32 = np.zeros(B, dtype=np.int32)
    i64 = np.zeros(B, dtype=np.int64)
    gamma = np.zeros(B)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lowpass = gpu.BatchLowpassProblem(n, *[np.full(B, v) for v in (0.12, 0.20, 0.5, 1.5, 0.3)])
    assert lib.ellhip_batch_lowpass_feas(batch._h, lowpass._h, 10, 1e-8, p(x), p(i32), p(i64), p(i32)) == capi.E_INVALID
    assert b"streamed" in lib.ellhip_last_error()
    f = rng.standard_normal((B, n, 2, 2))
    lmi = gpu.BatchLmiProblem([f + np.swapaxes(f, 2, 3)])
    assert lib.ellhip_batch_lmi_feas(batch._h, lmi._h, 10, 1e-8, p(x), p(i32), p(i64), p(i32)) == capi.E_INVALID
    assert b"streamed" in lib.ellhip_last_error()
    svm = gpu.BatchSvmProblem(rng.standard_normal((8, n - 1)), rng.choice([-1, 1], size=(B, 8)))
    assert lib.ellhip_batch_svm_optim(batch._h, svm._h, p(gamma), 10, 1e-8, p(x), p(i32), p(i64), p(i32)) == capi.E_INVALID
    assert b"streamed" in lib.ellhip_last_error()
    same_bits(batch.mq, before, "untouched")
