"""GPU: the EllStable variant of the batched small-n engine (include/ellhip_batch.h: ellhip_batch_create_stable,
ellhip_batch_stable_from_space) against the CPU oracle's EllStable (oracle/ell_oracle.c, orc_ellstable_update).  The
kernel follows EllStable::update_core statement for statement, so the comparison is EXACT: statuses, tsq, xc, kappa and
the whole packed buffer -- diagonal, factor and scratch triangle -- under np.array_equal (NaN masks compared)."""
import ctypes as C
import math

import numpy as np
import pytest

from pins import PINNED
from util import beta_of, mixed_cut, random_factor, set_default, stable_tau

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 7, 16, 33, 64, 65, 100, 128]
LAUNCHES = [1, 5, 8, 8, 1, 5]  # 28 cuts per ellipsoid
# several workgroups' worth of ellipsoids: up to 64 per one-wave workgroup at small n, one per workgroup from n = 64 up
POP = {1: 140, 2: 140, 3: 140, 7: 140, 16: 40, 33: 11}


def _orc_use_parallel_cut(orc, o, flag):
    """orc_ellstable has no setter for its EllCalc's flag: set it through the head of the struct (oracle/ell_oracle.h)."""
    class Head(C.Structure):
        _fields_ = [("n", C.c_int64), ("mq", C.c_void_p), ("xc", C.c_void_p), ("kappa", C.c_double),
                    ("tsq", C.c_double), ("corrected", C.c_int), ("helper", orc._Calc)]
    C.cast(C.c_void_p(o.h), C.POINTER(Head)).contents.helper.use_parallel_cut = int(flag)


def _make(gpu, orc, ctor, B, n, rng):
    xc0 = rng.standard_normal((B, n))
    if ctor == "matrix":  # random factor, junk in the scratch triangle
        kappa = 0.5 + 2.0 * rng.random(B)
        mq = np.stack([random_factor(n, int(rng.integers(1 << 30))) for _ in range(B)])
        return (gpu.EllStableBatch.new_with_matrix(kappa, mq, xc0),
                [orc.OracleEllStable.new_with_matrix(kappa[b], mq[b], xc0[b]) for b in range(B)])
    if ctor == "new":
        diag = 0.5 + rng.random((B, n))
        return gpu.EllStableBatch.new(diag, xc0), [orc.OracleEllStable.new(diag[b], xc0[b]) for b in range(B)]
    val = 0.5 + 2.0 * rng.random(B)
    return (gpu.EllStableBatch.new_with_scalar(val, xc0),
            [orc.OracleEllStable.new_with_scalar(val[b], xc0[b]) for b in range(B)])


def _cut(o, c, rng):
    """Cut number c of one ellipsoid: mixed_cut's eight forms (all six EllCalc entry points; NoSoln at c % 8 == 7) and a
    NoEffect cut (update_q with eta = tau + n beta < 0) at c % 11 == 10."""
    n = o.n
    g = rng.standard_normal(n)
    g /= np.linalg.norm(g)
    tau = stable_tau(o, g)
    if c % 11 == 10:
        return 2, g, -2.0 * tau / n, None
    kind, b0, b1 = mixed_cut(c, g, tau, rng)
    return kind, g, b0, b1


def _same_state(batch, ors, what=""):
    np.testing.assert_array_equal(batch.mq, np.stack([o.mq for o in ors]), err_msg=f"{what} mq")
    np.testing.assert_array_equal(batch.xc(), np.stack([np.array(o.xc) for o in ors]), err_msg=f"{what} xc")
    np.testing.assert_array_equal(batch.kappa, np.array([o.kappa for o in ors]), err_msg=f"{what} kappa")
    np.testing.assert_array_equal(batch.tsq(), np.array([o.tsq for o in ors]), err_msg=f"{what} tsq")


def _launch(batch, ors, K, c0, rng):
    """K cuts per ellipsoid (cut numbers c0 .. c0+K-1, shifted by b so that one launch mixes kinds and outcomes) on the
    batch in one launch and on the oracles one by one; statuses and tsq must agree exactly."""
    B, n = batch.B, batch.n
    kinds = np.zeros((K, B), dtype=np.int32)
    grads = np.zeros((K, B, n))
    b0 = np.zeros((K, B))
    b1 = np.full((K, B), np.nan)
    want = np.zeros((K, B), dtype=np.int32)
    want_tsq = np.zeros((K, B))
    for k in range(K):
        for b, o in enumerate(ors):
            kind, g, c_0, c_1 = _cut(o, c0 + k + b, rng)
            kinds[k, b], grads[k, b], b0[k, b] = kind, g, c_0
            if c_1 is not None:
                b1[k, b] = c_1
            want[k, b] = o.update(kind, g, c_0, c_1)
            want_tsq[k, b] = o.tsq
    status, tsq = batch.update(kinds, grads, b0, b1)
    np.testing.assert_array_equal(status, want)
    np.testing.assert_array_equal(tsq, want_tsq)
    return status


def _drive(gpu, orc, n, ctor="matrix", use_parallel=True, seed=0, B=None):
    rng = np.random.default_rng(seed)
    B = B or POP.get(n, 3)
    batch, ors = _make(gpu, orc, ctor, B, n, rng)
    assert batch.variant == gpu.capi.SPACE_ELL_STABLE
    if not use_parallel:
        batch.set_use_parallel_cut(False)
        for o in ors:
            _orc_use_parallel_cut(orc, o, 0)
    counts = np.zeros(4, dtype=int)
    c = 0
    for K in LAUNCHES:
        counts += np.bincount(_launch(batch, ors, K, c, rng).ravel(), minlength=4)
        c += K
        _same_state(batch, ors, what=f"n={n} after {c} cuts")
    return batch, ors, counts


@pytest.mark.parametrize("n", SIZES)
def test_bit_exact_against_oracle_on_random_factors(gpu, orc, n):
    batch, _, counts = _drive(gpu, orc, n, seed=4000 + n)
    if n > 1:
        assert counts[0] > counts[1:].sum() and counts[1] > 0 and counts[2] > 0, counts
        m = batch.mq
        if n > 2:  # not a comparison of zeros: factor and scratch triangle are populated
            assert np.count_nonzero(np.triu(m, 1)) >= batch.B * (n * (n - 1) // 2) * 9 // 10
            assert np.count_nonzero(np.tril(m, -1)) >= batch.B * (n * (n - 1) // 2) * 9 // 10


@pytest.mark.parametrize("n", [2, 16, 65, 128])
def test_bit_exact_without_parallel_cuts(gpu, orc, n):
    _drive(gpu, orc, n, use_parallel=False, seed=5000 + n)


@pytest.mark.parametrize("ctor", ["new", "scalar"])
@pytest.mark.parametrize("n", [1, 3, 16, 128])
def test_bit_exact_from_each_constructor(gpu, orc, n, ctor):
    _drive(gpu, orc, n, ctor=ctor, seed=6000 + n)


@pytest.mark.parametrize("solve", [0, 3])
@pytest.mark.parametrize("n", [12, 96])
def test_from_space_clones_an_ellstable_handle(gpu, orc, n, solve):
    set_default("STABLE_SOLVE", solve)
    rng = np.random.default_rng(70 + n + solve)
    f = random_factor(n, 80 + n)
    xc0 = np.linspace(-1.0, 1.0, n)
    space = gpu.EllStable.new_with_matrix(1.5, f, xc0)
    twin = gpu.EllStable.new_with_matrix(1.5, f, xc0)
    o = orc.OracleEllStable.new_with_matrix(1.5, f, xc0)
    statuses = []
    for c in (0, 2, 7, 4, 5, 1, 3):  # a failing cut (NoSoln) in the middle
        kind, g, b0, b1 = _cut(o, c, rng)
        statuses.append(o.update(kind, g, b0, b1))
        for s in (space, twin):
            assert int(s._update(kind, (g, beta_of(b0, b1)))) == statuses[-1]
    assert 1 in statuses
    assert twin.get_option(gpu.capi.OPT_STABLE_SOLVE) == solve
    twin_mq = twin.mq  # what observing the buffer does to a handle (the mirrored layout is left)
    B = 5
    batch = gpu.EllStableBatch.from_space(space, B)
    assert (batch.B, batch.n, batch.variant) == (B, n, gpu.capi.SPACE_ELL_STABLE)
    src_mq, src_xc = space.mq, space.xc()
    assert np.array_equal(src_mq, twin_mq)
    np.testing.assert_array_equal(batch.mq, np.broadcast_to(src_mq, (B, n, n)))
    np.testing.assert_array_equal(batch.xc(), np.broadcast_to(src_xc, (B, n)))
    np.testing.assert_array_equal(batch.kappa, np.full(B, space.kappa))
    np.testing.assert_array_equal(batch.tsq(), np.full(B, space.tsq()))
    # the source's next cut is the one an observed twin makes
    kind, g, b0, b1 = _cut(o, 0, rng)
    assert int(space._update(kind, (g, beta_of(b0, b1)))) == int(twin._update(kind, (g, beta_of(b0, b1))))
    assert np.array_equal(space.mq, twin.mq) and np.array_equal(space.xc(), twin.xc())
    assert space.kappa == twin.kappa and space.tsq() == twin.tsq()
    # every clone goes on exactly like an oracle space seeded from the cloned buffer
    ors = [orc.OracleEllStable.new_with_matrix(float(batch.kappa[b]), src_mq, src_xc) for b in range(B)]
    c = 0
    for K in (5, 1, 8):
        _launch(batch, ors, K, c, rng)
        c += K
        _same_state(batch, ors, what=f"clones after {c} cuts")
    with pytest.raises(gpu.capi.EllHipError):
        gpu.EllStableBatch.from_space(gpu.Ell.new_with_scalar(1.0, np.zeros(n)), 2)


class QuasiCvx:
    """src/quasicvx.rs:17-51 (tests/cpp/example_oracles.hpp: QuasiCvx): max sqrt(x)/y in log variables."""

    def __init__(self):
        self.idx = -1

    def assess_optim(self, xc, gamma):
        sqrtx, logy = float(xc[0]), float(xc[1])
        for _ in range(2):
            self.idx = 0 if self.idx + 1 == 2 else self.idx + 1
            if self.idx == 0:
                fv = sqrtx * sqrtx - logy
                if fv > 0.0:
                    return (np.array([2.0 * sqrtx, -1.0]), fv), False, gamma
            else:
                fv = -sqrtx + gamma * math.exp(logy)
                if fv > 0.0:
                    return (np.array([-1.0, gamma * math.exp(logy)]), fv), False, gamma
        return (np.array([-1.0, sqrtx]), 0.0), True, sqrtx / math.exp(logy)


# src/quasicvx.rs:101-133: (name, constructor, gamma0, max_iters, tolerance)
QUASICVX_STABLE = [("quasicvx_feasible_stable", ("new", [10.0, 10.0], [0.0, 0.0]), 0.0, 2000, 1e-8),
                   ("quasicvx_infeasible1_stable", ("scalar", 10.0, [100.0, 100.0]), 0.0, 2000, 1e-20),
                   ("quasicvx_infeasible2_stable", ("new", [10.0, 10.0], [0.0, 0.0]), 100.0, 2000, 1e-20)]


def test_reference_quasicvx_cases_side_by_side(gpu, orc):
    """The three EllStable cases in one batch (one launch per round, each space with its own cut kind; a finished case
    receives a failing cut, beta = +inf), decision for decision the three oracle loops (cutting_plane_optim,
    src/cutting_plane.rs:286-313), and the pinned outcomes."""
    def ctor(cls, spec):
        kind, a, xc = spec
        return cls.new(np.array(a), np.array(xc)) if kind == "new" else cls.new_with_scalar(a, np.array(xc))

    want = []
    for name, spec, gamma, max_iters, tol in QUASICVX_STABLE:
        o, ask, x_best, trace, niter_out = ctor(orc.OracleEllStable, spec), QuasiCvx(), None, [], max_iters
        for niter in range(max_iters):
            x = np.array(o.xc)
            (g, beta), shrunk, gamma = ask.assess_optim(x, gamma)
            if shrunk:
                x_best = x
            st = o.update(1 if shrunk else 0, g, beta)
            trace.append((shrunk, st, o.tsq))
            if st != 0 or o.tsq < tol:
                niter_out = niter
                break
        want.append((x_best, niter_out, gamma, trace))
    B, n = len(QUASICVX_STABLE), 2
    kappa = np.array([1.0 if s[0] == "new" else s[1] for _, s, *_ in QUASICVX_STABLE])
    mq = np.stack([np.diag(s[1]) if s[0] == "new" else np.eye(n) for _, s, *_ in QUASICVX_STABLE])
    batch = gpu.EllStableBatch.new_with_matrix(kappa, mq, np.array([s[2] for _, s, *_ in QUASICVX_STABLE]))
    asks = [QuasiCvx() for _ in range(B)]
    gamma = [c[2] for c in QUASICVX_STABLE]
    x_best, traces, niter_out, done = [None] * B, [[] for _ in range(B)], [c[3] for c in QUASICVX_STABLE], [False] * B
    for it in range(max(c[3] for c in QUASICVX_STABLE)):
        if all(done):
            break
        xc = batch.xc()
        kinds, grads, beta = np.zeros(B, dtype=np.int32), np.ones((B, n)), np.full(B, np.inf)
        shrunk = [False] * B
        for b in range(B):
            if not done[b]:
                (g, bt), shrunk[b], gamma[b] = asks[b].assess_optim(xc[b], gamma[b])
                if shrunk[b]:
                    x_best[b] = xc[b].copy()
                kinds[b], grads[b], beta[b] = (1 if shrunk[b] else 0), g, bt
        status, tsq = batch.update(kinds, grads, beta)
        for b in range(B):
            if not done[b]:
                traces[b].append((shrunk[b], int(status[0, b]), float(tsq[0, b])))
                if status[0, b] != 0 or tsq[0, b] < QUASICVX_STABLE[b][4]:
                    done[b], niter_out[b] = True, it
    for b, (name, *_rest) in enumerate(QUASICVX_STABLE):
        xb, ni, gm, trace = want[b]
        assert traces[b] == trace, name
        assert niter_out[b] == ni and gamma[b] == gm, name
        assert (x_best[b] is None) == (xb is None) and (xb is None or np.array_equal(x_best[b], xb)), name
        pinned_niter, has_x, _, _ = PINNED[name]
        assert (x_best[b] is not None) == has_x, name
        if pinned_niter is not None:
            assert niter_out[b] == pinned_niter, name


def test_large_population_is_exact(gpu, orc):
    """20 000 ellipsoids of n = 16 (1334 workgroups), 4 cuts each in one launch, against 20 000 oracle spaces."""
    B, n, K = 20000, 16, 4
    rng = np.random.default_rng(12)
    f = random_factor(n, 13)
    xc0 = rng.standard_normal((B, n))
    batch = gpu.EllStableBatch.new_with_matrix(1.0, np.broadcast_to(f, (B, n, n)), xc0)
    ors = [orc.OracleEllStable.new_with_matrix(1.0, f, xc0[b]) for b in range(B)]
    grads = rng.standard_normal((K, B, n))
    kinds = rng.integers(0, 2, (K, B)).astype(np.int32)
    beta = 0.01 * rng.random((K, B))
    want = np.array([[o.update(int(kinds[k, b]), grads[k, b], float(beta[k, b])) for b, o in enumerate(ors)]
                     for k in range(K)])
    status, _ = batch.update(kinds, grads, beta)
    np.testing.assert_array_equal(status, want)
    assert np.count_nonzero(status == 0) > K * B * 9 // 10
    _same_state(batch, ors)


def test_ell_and_ellstable_batches_alternate(gpu, orc):
    """The two kernels' dynamic-LDS opt-ins are their own: an Ell batch at n = 100 (~80 KiB) and EllStable batches at
    n = 8 (a few KiB) and n = 128 (133 KiB), launched in turn, all stay exact."""
    rng = np.random.default_rng(21)
    ell = gpu.EllBatch.new_with_scalar(np.ones(3), np.zeros((3, 100)))
    ell_o = [orc.OracleEll.new_with_scalar(1.0, np.zeros(100)) for _ in range(3)]
    pops = [(ell, ell_o)]
    for n, B in ((8, 70), (128, 2)):
        pops.append(_make(gpu, orc, "matrix", B, n, rng))
    c = 0
    for _ in range(2):
        for batch, ors in pops:
            if batch.variant == gpu.capi.SPACE_ELL:
                g = rng.standard_normal((2, batch.B, batch.n))
                st, _ = batch.update(np.zeros((2, batch.B), dtype=np.int32), g, np.full((2, batch.B), 0.01))
                want = [[o.update(0, g[k, b], 0.01) for b, o in enumerate(ors)] for k in range(2)]
                np.testing.assert_array_equal(st, want)
            else:
                _launch(batch, ors, 3, c, rng)
            _same_state(batch, ors)
        c += 3


def _hip(gpu):
    """The HIP runtime the engine is bound to (the package may have opened PyTorch-ROCm's copy, capi.load)."""
    paths = sorted(gpu.capi.mapped_runtimes()["libamdhip64"])
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_update_dev_gives_the_bits_of_update(gpu, orc):
    """The same cuts through ellhip_batch_update_dev (arrays already in HBM) and ellhip_batch_update."""
    n, B, K = 16, 33, 5
    rng = np.random.default_rng(31)
    f = random_factor(n, 32)
    xc0 = rng.standard_normal((B, n))
    a = gpu.EllStableBatch.new_with_matrix(1.0, np.broadcast_to(f, (B, n, n)), xc0)
    d = gpu.EllStableBatch.new_with_matrix(1.0, np.broadcast_to(f, (B, n, n)), xc0)
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
    np.testing.assert_array_equal(outs[1], ts_a)
    for get in ("mq", "kappa"):
        np.testing.assert_array_equal(getattr(d, get), getattr(a, get))
    np.testing.assert_array_equal(d.xc(), a.xc())
    np.testing.assert_array_equal(d.tsq(), a.tsq())


def test_argument_checks_and_variant(gpu):
    lib = gpu.capi.load()
    with pytest.raises(gpu.capi.EllHipError):
        gpu.EllStableBatch.new_with_scalar(np.ones(2), np.zeros((2, 129)))
    s = gpu.EllStableBatch.new_with_scalar(1.0, np.zeros((2, 4)))
    e = gpu.EllBatch.new_with_scalar(1.0, np.zeros((2, 4)))
    assert (s.variant, e.variant) == (gpu.capi.SPACE_ELL_STABLE, gpu.capi.SPACE_ELL)
    assert not hasattr(s, "set_no_defer_trick")
    assert lib.ellhip_batch_set_no_defer_trick(s._h, 1) == gpu.capi.E_INVALID
    assert lib.ellhip_batch_set_no_defer_trick(e._h, 0) == 0
    with pytest.raises(gpu.capi.EllHipError):
        s.update(np.full(2, 7, dtype=np.int32), np.zeros((2, 4)), np.zeros(2))
    with pytest.raises(gpu.capi.EllHipError):
        gpu.EllBatch.from_space(gpu.EllStable.new_with_scalar(1.0, np.zeros(4)), 3)


def test_cpp_mirror_runs_the_quasicvx_cases(gpu):
    import cpp_build
    exe = cpp_build.build_runner("batch_stable_runner.cpp", "hip")
    res = cpp_build.run_json_lines(exe)
    assert sorted(res) == sorted(c[0] for c in QUASICVX_STABLE)
    for name, r in res.items():
        # batched engine (bit-exact CPU order) vs one EllStableHip handle each (the 1e-10 parity engine)
        assert r["niter_batch"] == r["niter_single"], r
        assert r["has_x_batch"] == r["has_x_single"] == PINNED[name][1], r
        assert abs(r["gamma_batch"] - r["gamma_single"]) <= 1e-9 * max(1.0, abs(r["gamma_single"])), r
        assert r["max_dx"] <= 1e-9, r
