"""GPU: EllStable on the streamed batch engine (include/ellhip_batch_streamed_stable.h) against the CPU oracle's EllStable,
against the LDS EllStable engine and against itself across launch splits, through the C ABI.  The engine follows
EllStable::update_core statement for statement, so every comparison is on bit patterns -- statuses, tsq, xc, kappa and the
whole packed buffer, scratch triangle included -- with NaNs compared by position (the payload of a NaN is not part of the
reference's contract)."""
import ctypes as C

import numpy as np
import pytest

from numeric_edges import SCALE_EXPONENTS, mixed_seq, oracle_run, scaled, subnormal_seq, with_zero
from util import mixed_cut, random_factor, stable_tau

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


def assert_same_batches(a, b, what=""):
    same_bits(a.mq, b.mq, what + " mq")
    same_bits(a.xc(), b.xc(), what + " xc")
    same_bits(a.kappa, b.kappa, what + " kappa")
    same_bits(a.tsq(), b.tsq(), what + " tsq")


def apply_cuts(batch, ors, kinds, grads, b0, b1):
    """One launch of K cuts on the batch, the same cuts one by one on the oracles; every status and tsq compared.
    kinds, b0, b1: [K][B] (b1 NaN = no second value), grads [K][B][n].  Returns the statuses."""
    K, B = kinds.shape
    want = np.zeros((K, B), dtype=np.int32)
    want_tsq = np.zeros((K, B))
    for k in range(K):
        for b, o in enumerate(ors):
            want[k, b] = o.update(int(kinds[k, b]), grads[k, b], float(b0[k, b]),
                                  None if np.isnan(b1[k, b]) else float(b1[k, b]))
            want_tsq[k, b] = o.tsq
    status, tsq = batch.update(kinds, grads, b0, b1)
    np.testing.assert_array_equal(status, want)
    same_bits(tsq, want_tsq, "tsq per cut")
    return status


def mixed_round(ors, K, n, rng, it):
    """K mixed cuts per ellipsoid (tests/util.py: mixed_cut), beta scaled by the tau each oracle sees at the START of the round
    (tests/util.py: stable_tau, from a clone): the oracles are not advanced here, apply_cuts does that."""
    B = len(ors)
    kinds = np.zeros((K, B), dtype=np.int32)
    grads = rng.standard_normal((K, B, n))
    b0 = np.zeros((K, B))
    b1 = np.full((K, B), np.nan)
    for b, o in enumerate(ors):
        for k in range(K):
            kind, c0, c1 = mixed_cut(it + k + b, grads[k, b], stable_tau(o, grads[k, b]), rng)
            kinds[k, b], b0[k, b] = kind, c0
            if c1 is not None:
                b1[k, b] = c1
    return kinds, grads, b0, b1


def make(gpu, orc, B, n, rng, *, matrix=False):
    kappa = 0.5 + 2.0 * rng.random(B)
    xc0 = rng.standard_normal((B, n))
    if matrix:  # random positive diagonal, random strict upper factor, random strict lower triangle
        mq = np.stack([random_factor(n, int(rng.integers(1 << 30))) for _ in range(B)])
        batch = gpu.EllStableBatchStreamed.new_with_matrix(kappa, mq, xc0)
        return batch, [orc.OracleEllStable.new_with_matrix(kappa[b], mq[b], xc0[b]) for b in range(B)], mq
    batch = gpu.EllStableBatchStreamed.new_with_scalar(kappa, xc0)
    return batch, [orc.OracleEllStable.new_with_scalar(kappa[b], xc0[b]) for b in range(B)], None


def check_handle(gpu, batch, B, n):
    assert batch.is_streamed and batch.variant == gpu.capi.SPACE_ELL_STABLE and (batch.B, batch.n) == (B, n)


def cuts(rng, B, n, spec):
    """spec: one (kind, beta0, beta1) per cut of the launch, the same for every ellipsoid; fresh normal gradients"""
    K = len(spec)
    kinds = np.array([[s[0]] * B for s in spec], dtype=np.int32)
    b0 = np.array([[s[1]] * B for s in spec], dtype=np.float64)
    b1 = np.array([[s[2]] * B for s in spec], dtype=np.float64)
    return kinds, rng.standard_normal((K, B, n)), b0, b1


OK_CUT = (0, 0.01, np.nan)
NOSOLN = (0, np.inf, np.nan)
NOEFFECT = (2, -1e3, np.nan)   # a q-cut far on the other side of the centre (tau + n * beta < 0, EllCalc::calc_bias_cut_q)


# ---- 1. exact against the CPU oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 191, 192, 193, 257, 512, 1000, 1023, 1024])
def test_bit_identical_to_the_oracle(gpu, orc, n):
    """B = 3, K = 3, two rounds, from random factors: from the identity the reference's factor stays the identity (its
    update multiplies the factor's own elements), and the comparison would be one of zeros.  Every seed gives Success and
    NoSoln cuts (checked on the oracle alone)."""
    B, K = 3, 3
    rng = np.random.default_rng(2000 + n)
    batch, ors, _ = make(gpu, orc, B, n, rng, matrix=True)
    check_handle(gpu, batch, B, n)
    counts = np.zeros(4, dtype=int)
    for r in range(2):
        counts += np.bincount(apply_cuts(batch, ors, *mixed_round(ors, K, n, rng, r * K)).ravel(), minlength=4)
    assert_state(batch, ors)
    assert counts[0] > 0
    m = batch.mq   # not a comparison of zeros: factor and scratch triangle are populated
    assert np.count_nonzero(np.triu(m, 1)) >= B * (n * (n - 1) // 2) * 9 // 10
    assert np.count_nonzero(np.tril(m, -1)) >= B * (n * (n - 1) // 2) * 9 // 10


# ---- 2. the caller's matrix ------------------------------------------------------------------------------------------------
def test_the_callers_matrix_comes_back_and_is_used(gpu, orc):
    B, n, K = 3, 130, 3
    rng = np.random.default_rng(21)
    batch, ors, mq = make(gpu, orc, B, n, rng, matrix=True)
    check_handle(gpu, batch, B, n)
    assert np.count_nonzero(np.tril(mq, -1)) == B * n * (n - 1) // 2
    same_bits(batch.mq, mq, "mq as given")
    same_bits(batch.mq, mq, "mq as given, read twice")
    seen = 0
    for r in range(2):
        seen += int((apply_cuts(batch, ors, *mixed_round(ors, K, n, rng, r * K)) == 0).sum())
    assert seen > 0
    assert_state(batch, ors)


# ---- 3. failed cuts ----------------------------------------------------------------------------------------------------------
def test_a_failed_cut_changes_tsq_and_scratch_only(gpu, orc):
    B, n = 2, 130
    rng = np.random.default_rng(33)
    batch, ors, _ = make(gpu, orc, B, n, rng, matrix=True)
    spec = [OK_CUT, NOSOLN, OK_CUT, NOEFFECT, OK_CUT]
    kinds, grads, b0, b1 = cuts(rng, B, n, spec)
    got = []
    for k in range(len(spec)):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        status = apply_cuts(batch, ors, kinds[k:k + 1], grads[k:k + 1], b0[k:k + 1], b1[k:k + 1])
        got.append(int(status[0, 0]))
        assert np.all(status == status[0, 0])
        assert_state(batch, ors, f"after cut {k}")
        if status[0, 0] != 0:
            mq = batch.mq
            for b in range(B):
                same_bits(np.triu(mq[b]), np.triu(before[0][b]), "diagonal and factor after a failed cut")
                assert not np.array_equal(np.tril(mq[b], -1), np.tril(before[0][b], -1))   # the forward solve ran
            same_bits(batch.xc(), before[1], "xc after a failed cut")
            same_bits(batch.kappa, before[2], "kappa after a failed cut")
            assert not np.array_equal(batch.tsq(), before[3])
    assert got == [0, 1, 0, 2, 0]


# ---- 4. exact against the LDS EllStable engine -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 63, 64, 65, 128])
def test_equals_the_lds_engine(gpu, orc, n):
    B, K = 37, 4
    rng = np.random.default_rng(300 + n)
    kappa = 0.5 + 2.0 * rng.random(B)
    xc0 = rng.standard_normal((B, n))
    mq = np.stack([random_factor(n, 900 + n + b) for b in range(B)])
    lds = gpu.EllStableBatch.new_with_matrix(kappa, mq, xc0)
    st = gpu.EllStableBatchStreamed.new_with_matrix(kappa, mq, xc0)
    check_handle(gpu, st, B, n)
    same_bits(st.mq, mq, "mq as given")
    seen = np.zeros(4, dtype=int)
    for r in range(3):
        # tau from the LDS engine's own answer to a central cut on a copy of its state at the start of the round: tsq = tau^2
        kap_r, mq_r, xc_r = lds.kappa, lds.mq, lds.xc()
        grads = rng.standard_normal((K, B, n))
        kinds = np.zeros((K, B), dtype=np.int32)
        b0 = np.zeros((K, B))
        b1 = np.full((K, B), np.nan)
        for k in range(K):
            _, tsq = gpu.EllStableBatch.new_with_matrix(kap_r, mq_r, xc_r).update(np.ones(B, dtype=np.int32), grads[k], np.zeros(B))
            with np.errstate(invalid="ignore"):  # n = 1: kappa turns inf (cst1 = inf) and tsq NaN
                tau = np.sqrt(np.maximum(tsq[0], 0.0))
            for b in range(B):
                kind, c0, c1 = mixed_cut(r * K + k + b, grads[k, b], tau[b], rng)
                kinds[k, b], b0[k, b] = kind, c0
                if c1 is not None:
                    b1[k, b] = c1
        status_s, tsq_s = st.update(kinds, grads, b0, b1)
        status_l, tsq_l = lds.update(kinds, grads, b0, b1)
        np.testing.assert_array_equal(status_s, status_l)
        same_bits(tsq_s, tsq_l, "tsq per cut")
        seen += np.bincount(status_l.ravel(), minlength=4)
        assert_same_batches(st, lds, f"round {r}")
    assert seen[0] > 0 and seen[1:].sum() > 0


# ---- 5. launch splitting -----------------------------------------------------------------------------------------------------
def test_one_launch_of_six_equals_six_launches_of_one(gpu, orc):
    B, n = 3, 192
    rng = np.random.default_rng(55)
    kappa = 0.5 + 2.0 * rng.random(B)
    xc0 = rng.standard_normal((B, n))
    mq = np.stack([random_factor(n, 56 + b) for b in range(B)])
    one = gpu.EllStableBatchStreamed.new_with_matrix(kappa, mq, xc0)
    six = gpu.EllStableBatchStreamed.new_with_matrix(kappa, mq, xc0)
    kinds, grads, b0, b1 = cuts(rng, B, n, [OK_CUT, (1, 0.0, 0.3), NOSOLN, OK_CUT, (2, 0.005, np.nan), (0, 0.02, np.nan)])
    st6, ts6 = six.update(kinds, grads, b0, b1)
    for k in range(6):
        st1, ts1 = one.update(kinds[k], grads[k], b0[k], b1[k:k + 1])
        np.testing.assert_array_equal(st1[0], st6[k])
        same_bits(ts1[0], ts6[k], "tsq")
    assert st6[:, 0].tolist() == [0, 0, 1, 0, 0, 0]
    assert_same_batches(one, six)


# ---- 6. clones ---------------------------------------------------------------------------------------------------------------
def test_from_space_clones_an_ellstable_handle(gpu, orc):
    n, B = 200, 4
    rng = np.random.default_rng(66)
    base = gpu.EllStable.new_with_matrix(1.5, random_factor(n, 67), np.linspace(-1.0, 1.0, n))
    for _ in range(5):
        g = rng.standard_normal(n)
        assert int(base._update(0, (g, 0.01))) == 0
    batch = gpu.EllStableBatchStreamed.from_space(base, B)
    check_handle(gpu, batch, B, n)
    src_mq, src_xc = base.mq, base.xc()
    assert np.count_nonzero(np.tril(src_mq, -1)) > 0
    same_bits(batch.mq, np.broadcast_to(src_mq, (B, n, n)), "clones")
    same_bits(batch.xc(), np.broadcast_to(src_xc, (B, n)), "clones xc")
    same_bits(batch.kappa, np.full(B, base.kappa), "clones kappa")
    same_bits(batch.tsq(), np.full(B, base.tsq()), "clones tsq")
    ors = [orc.OracleEllStable.new_with_matrix(base.kappa, src_mq, src_xc) for _ in range(B)]
    seen = 0
    for r in range(2):   # probes diverge from here: different cuts per clone
        seen += int((apply_cuts(batch, ors, *mixed_round(ors, 3, n, rng, 3 * r)) == 0).sum())
    assert seen > 0
    assert_state(batch, ors)
    assert not np.array_equal(batch.xc()[0], batch.xc()[1])


# ---- 7. options --------------------------------------------------------------------------------------------------------------
def _orc_use_parallel_cut(orc, o, flag):
    """orc_ellstable has no setter for its EllCalc's flag: set it through the head of the struct (oracle/ell_oracle.h)."""
    class Head(C.Structure):
        _fields_ = [("n", C.c_int64), ("mq", C.c_void_p), ("xc", C.c_void_p), ("kappa", C.c_double),
                    ("tsq", C.c_double), ("corrected", C.c_int), ("helper", orc._Calc)]
    C.cast(C.c_void_p(o.h), C.POINTER(Head)).contents.helper.use_parallel_cut = int(flag)


def test_use_parallel_cut_is_honoured_and_no_defer_trick_refused(gpu, orc):
    B, n = 3, 130
    rng = np.random.default_rng(77)
    batch, ors, _ = make(gpu, orc, B, n, rng, matrix=True)
    twin, twin_ors, _ = make(gpu, orc, B, n, np.random.default_rng(77), matrix=True)
    batch.set_use_parallel_cut(False)
    for o in ors:
        _orc_use_parallel_cut(orc, o, 0)
    # parallel cuts (both values given): with the flag off the second value is ignored, and the result differs
    kinds, grads, b0, b1 = cuts(rng, B, n, [(0, 0.01, 0.5), (1, 0.0, 0.4), (2, 0.01, 0.6)])
    assert np.all(apply_cuts(batch, ors, kinds, grads, b0, b1) == 0)
    assert np.all(apply_cuts(twin, twin_ors, kinds, grads, b0, b1) == 0)
    assert_state(batch, ors)
    assert_state(twin, twin_ors)
    assert not np.array_equal(batch.kappa, twin.kappa)
    lib = gpu.capi.load()
    assert not hasattr(batch, "set_no_defer_trick")
    assert lib.ellhip_batch_set_no_defer_trick(batch._h, 1) == gpu.capi.E_INVALID
    assert np.all(apply_cuts(batch, ors, *cuts(rng, B, n, [OK_CUT])) == 0)
    assert_state(batch, ors)


# ---- 8. _update_dev ----------------------------------------------------------------------------------------------------------
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
    mq = np.stack([random_factor(n, 32 + b) for b in range(B)])
    a = gpu.EllStableBatchStreamed.new_with_matrix(2.0, mq, xc0)
    d = gpu.EllStableBatchStreamed.new_with_matrix(2.0, mq, xc0)
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
        assert gpu.capi.load().ellhip_batch_stream(d._h)
        for p, x in zip(ptrs[len(host):], outs):
            assert hip.hipMemcpy(x.ctypes.data, p, x.nbytes, 2) == 0
    finally:
        for p in ptrs:
            hip.hipFree(p)
    np.testing.assert_array_equal(outs[0], st_a)
    same_bits(outs[1], ts_a, "tsq per cut")
    assert (st_a == 0).any()
    assert_same_batches(d, a)


# ---- 9. numeric edges (tests/numeric_edges.py) at n = 130 --------------------------------------------------------------------
EDGE_N, EDGE_B = 130, 4


def edge_run(gpu, orc, member_cuts):
    """Member b of one batch (kappa0 = 1, identity, xc0 = 0, as numeric_edges' sequences assume) takes member_cuts[b] in one
    launch; every member must be its own oracle run bit for bit.  Returns statuses, tsq [K][B] and the batch."""
    B = len(member_cuts)
    batch = gpu.EllStableBatchStreamed.new_with_scalar(1.0, np.zeros((B, EDGE_N)))
    kinds, grads, b0, b1 = (np.stack([c[f] for c in member_cuts], axis=1) for f in range(4))
    st, ts = batch.update(kinds, grads, b0, b1)
    ors = [orc.OracleEllStable.new_with_scalar(1.0, np.zeros(EDGE_N)) for _ in range(B)]
    for b, o in enumerate(ors):
        ost, ots = oracle_run(o, member_cuts[b])
        np.testing.assert_array_equal(st[:, b], ost)
        same_bits(ts[:, b], ots, f"member {b} tsq per cut")
    assert_state(batch, ors)
    return st, ts, batch


def test_zero_gradient_in_one_batch_member(gpu, orc):
    """Member 1 turns NaN at cut 3 (bias cut, beta = 0), member 2 meets a NoSoln zero cut at cut 5, member 3 a central zero
    cut at cut 2: every member -- the healthy one above all -- stays bit-identical to its own oracle run."""
    member_cuts = [mixed_seq(orc, EDGE_N, 10, 500 + 7 * b, stable=True) for b in range(EDGE_B)]
    member_cuts[1] = with_zero(member_cuts[1], [3], "nan")
    member_cuts[2] = with_zero(member_cuts[2], [5], "nosoln")
    member_cuts[3] = with_zero(member_cuts[3], [2], "central")
    st, ts, batch = edge_run(gpu, orc, member_cuts)
    assert st[3, 1] == 0 and ts[3, 1] == 0.0 and st[5, 2] == 1 and ts[5, 2] == 0.0 and st[2, 3] == 0 and ts[2, 3] == 0.0
    xc, mq = batch.xc(), batch.mq
    assert np.isnan(xc[1]).all() and np.isfinite(mq[0]).all() and np.isfinite(xc[0]).all() and np.isfinite(mq[2]).all()


def test_subnormal_omega(gpu, orc):
    st, ts, batch = edge_run(gpu, orc, [subnormal_seq(EDGE_N, seed=40 + b) for b in range(EDGE_B)])
    assert np.all(st == 0) and np.all(ts > 0.0) and np.all(ts < 1e-300)
    assert np.isfinite(batch.mq).all() and np.isfinite(batch.xc()).all()


def test_rescaled_run_is_the_same_run(gpu, orc):
    """(2^e g, 2^e beta): the same statuses, tsq times 4^e, and the same diagonal, factor, xc and kappa to the bit (the scratch
    triangle holds products with the gradient and scales with it); each run is also its own oracle run."""
    member_cuts = [mixed_seq(orc, EDGE_N, 10, 300 + 7 * b, stable=True) for b in range(EDGE_B)]
    st, ts, batch = edge_run(gpu, orc, member_cuts)
    assert (st == 0).any() and (st == 1).any()
    for e in SCALE_EXPONENTS:
        st2, ts2, batch2 = edge_run(gpu, orc, [scaled(c, e) for c in member_cuts])
        np.testing.assert_array_equal(st2, st)
        same_bits(ts2, ts * 4.0 ** e, f"tsq at 2^{e}")
        same_bits(np.triu(batch2.mq), np.triu(batch.mq), f"diagonal and factor at 2^{e}")
        same_bits(batch2.xc(), batch.xc(), f"xc at 2^{e}")
        same_bits(batch2.kappa, batch.kappa, f"kappa at 2^{e}")


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(gpu, orc):
    capi = gpu.capi
    lib = capi.load()
    h = C.c_void_p()
    for B, n in ((2, 0), (2, 1025), (0, 16)):
        assert lib.ellhip_batch_create_streamed_stable(C.byref(h), B, n, None, None, None, None, -1) == capi.E_INVALID
        assert not h.value
    with pytest.raises(capi.EllHipError):
        gpu.EllStableBatchStreamed.new_with_scalar(np.ones(2), np.zeros((2, 1025)))
    with pytest.raises(capi.EllHipError):
        gpu.EllStableBatch.new_with_scalar(np.ones(2), np.zeros((2, 129)))   # the LDS engine keeps its limit
    with pytest.raises(capi.EllHipError):
        gpu.EllStableBatchStreamed.from_space(gpu.Ell.new_with_scalar(1.0, np.zeros(4)), 3)
    with pytest.raises(capi.EllHipError):
        gpu.EllBatchStreamed.from_space(gpu.EllStable.new_with_scalar(1.0, np.zeros(4)), 3)
    assert lib.ellhip_batch_streamed_stable_from_space(C.byref(h), None, 3) == capi.E_INVALID and not h.value
    assert lib.ellhip_batch_is_streamed(gpu.EllStableBatch.new_with_scalar(1.0, np.zeros((2, 4)))._h) == 0
    # after all of that a good handle still runs
    n, B = 130, 2
    rng = np.random.default_rng(9)
    batch, ors, _ = make(gpu, orc, B, n, rng, matrix=True)
    assert np.all(apply_cuts(batch, ors, *cuts(rng, B, n, [OK_CUT, OK_CUT])) == 0)
    assert_state(batch, ors)


def test_every_batched_loop_refuses_the_handle_and_leaves_it_untouched(gpu, orc):
    """also at n <= 128, where the shapes would match: the LDS loops, their _stable forms and the streamed low-pass loops"""
    capi = gpu.capi
    lib = capi.load()
    n, B = 16, 2
    rng = np.random.default_rng(2)
    kappa = np.full(B, 40.0)
    mq = np.stack([random_factor(n, 5 + b) for b in range(B)])
    batch = gpu.EllStableBatchStreamed.new_with_matrix(kappa, mq, np.zeros((B, n)))
    ors = [orc.OracleEllStable.new_with_matrix(kappa[b], mq[b], np.zeros(n)) for b in range(B)]
    assert np.all(apply_cuts(batch, ors, *cuts(rng, B, n, [OK_CUT])) == 0)
    before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
    x = np.zeros((B, n))
    i32 = np.zeros(B, dtype=np.int32)
    i64 = np.zeros(B, dtype=np.int64)
    gamma = np.zeros(B)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    spec = [np.full(B, v) for v in (0.12, 0.20, 0.5, 1.5, 0.3)]
    lowpass = gpu.BatchLowpassProblem(n, *spec)
    lowpass_streamed = gpu.BatchLowpassProblem.streamed(n, *spec)
    f = rng.standard_normal((B, n, 2, 2))
    lmi = gpu.BatchLmiProblem([f + np.swapaxes(f, 2, 3)])
    lmi_c = gpu.BatchLmiProblem([f + np.swapaxes(f, 2, 3)], c=rng.standard_normal((B, n)))
    svm = gpu.BatchSvmProblem(rng.standard_normal((8, n - 1)), rng.choice([-1, 1], size=(B, 8)))
    optim = lambda name, prob: getattr(lib, name)(batch._h, prob._h, p(gamma), 10, 1e-8, p(x), p(i32), p(i64), p(i32))
    feas = lambda name, prob: getattr(lib, name)(batch._h, prob._h, 10, 1e-8, p(x), p(i32), p(i64), p(i32))
    calls = [(feas, "ellhip_batch_lowpass_feas", lowpass), (optim, "ellhip_batch_lowpass_optim", lowpass),
             (feas, "ellhip_batch_lmi_feas", lmi), (optim, "ellhip_batch_lmi_optim", lmi_c),
             (optim, "ellhip_batch_svm_optim", svm),
             (feas, "ellhip_batch_lowpass_feas_stable", lowpass), (optim, "ellhip_batch_lowpass_optim_stable", lowpass),
             (feas, "ellhip_batch_lmi_feas_stable", lmi), (optim, "ellhip_batch_lmi_optim_stable", lmi_c),
             (optim, "ellhip_batch_svm_optim_stable", svm),
             (feas, "ellhip_batch_lowpass_feas_streamed", lowpass_streamed),
             (optim, "ellhip_batch_lowpass_optim_streamed", lowpass_streamed)]
    for call, name, prob in calls:
        assert call(name, prob) == capi.E_INVALID, name
        msg = lib.ellhip_last_error()
        assert b"streamed" in msg or b"EllStable" in msg, (name, msg)
        for got, want, what in zip((batch.mq, batch.xc(), batch.kappa, batch.tsq()), before, ("mq", "xc", "kappa", "tsq")):
            same_bits(got, want, f"{what} after {name}")
    assert_state(batch, ors)
    assert np.all(apply_cuts(batch, ors, *cuts(rng, B, n, [OK_CUT])) == 0)
    assert_state(batch, ors)
