"""GPU: the device-side SvmOracle (include/ellhip_svm.h) against the reference's SvmOracle restated in
tests/svm_reference.py, and its device-resident cutting_plane_optim against the host-driven loop (bit for bit, same
handle type and depth) and against the reference loop over the CPU oracle (niter and chosen samples exactly, state
within the suite's 1e-10).

The margins, the chosen sample, the gradient and beta / gamma are the reference's to the bit: every comparison below
looks at the bit patterns (so the sign of zero counts); NaN is compared by position."""
import ctypes as C

import numpy as np
import pytest

import svm_reference as ref
from util import TOL, rel_inf

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def clouds(m, nfeat, shift, seed):
    """two clouds around +-shift on feature 0, labels -1 for every third sample, +1 otherwise"""
    rng = np.random.default_rng(seed)
    lab = np.where(np.arange(m) % 3 == 0, -1, 1).astype(np.int32)
    X = rng.random((m, nfeat)) - 0.5
    X[:, 0] += shift * lab
    return X, lab


def check_assess(o, X, lab, x):
    (g, cut), shrunk, gamma = o.assess_optim(x, 123.0)
    (rg, rb), _, rgamma, ridx, rval = ref.assess_optim(X, lab, x)
    assert shrunk is True
    idx, val = o.last()
    assert idx == ridx and same_bits(val, rval), (idx, val, ridx, rval)
    assert same_bits(g, rg) and same_bits(cut.beta, rb) and same_bits(gamma, rgamma)
    return idx, val


# ---- margins, bit for bit -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,nfeat", [(1, 1), (2, 1), (7, 3), (513, 1), (1001, 17), (1537, 64), (4097, 2999),
                                     (131075, 260)])   # the last one is a 272 MB table, beyond the Infinity Cache
def test_margins_bit_for_bit(gpu, m, nfeat):
    rng = np.random.default_rng(m * 7 + nfeat)
    X = rng.standard_normal((m, nfeat))
    lab = rng.choice(np.array([-7, -1, 0, 1, 7], dtype=np.int32), size=m)
    o = gpu.SvmOracle(X, lab)
    for _ in range(2):
        x = rng.standard_normal(nfeat + 1)
        assert same_bits(o.margins(x), ref.margins(X, lab, x))
        check_assess(o, X, lab, x)


def test_margins_special_values(gpu):
    m, nfeat = 1031, 9
    rng = np.random.default_rng(5)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-310, -2.5])
    X = rng.choice(specials, size=(m, nfeat), p=[0.2, 0.2, 0.03, 0.03, 0.02, 0.2, 0.2, 0.05, 0.07])
    lab = rng.choice(np.array([-7, -1, 0, 1, 7], dtype=np.int32), size=m)
    o = gpu.SvmOracle(X, lab)
    for x in (np.zeros(nfeat + 1), np.full(nfeat + 1, -0.0), rng.choice(specials[[0, 1, 5, 6, 8]], size=nfeat + 1),
              np.where(rng.random(nfeat + 1) < 0.5, -0.0, 0.0)):
        mg = o.margins(x)
        assert same_bits(mg, ref.margins(X, lab, x))
        assert np.isnan(mg).any() and (mg == 0).any()
        check_assess(o, X, lab, x)


# ---- assess_optim -------------------------------------------------------------------------------------------------

def test_assess_optim_duplicates_and_ties(gpu):
    # duplicate rows: the first index wins
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5000, 11))
    lab = np.ones(5000, dtype=np.int32)
    x = rng.standard_normal(12)
    r = ref.argmin(ref.margins(X, lab, x))[0]
    X[4321] = X[r]
    X[r + 1 if r + 1 < 4321 else 0] = X[r]
    o = gpu.SvmOracle(X, lab)
    assert check_assess(o, X, lab, x)[0] == min(r, r + 1 if r + 1 < 4321 else 0)
    # -0.0 / +0.0 ties: the first index keeps its own sign; every other margin is 5
    for first, second in ((-1, 1), (1, -1)):
        X = np.full((600, 1), 5.0)
        lab = np.ones(600, dtype=np.int32)
        X[300, 0] = X[517, 0] = 0.0
        lab[300], lab[517] = first, second
        o = gpu.SvmOracle(X, lab)
        idx, val = check_assess(o, X, lab, np.array([1.0, 0.0]))
        assert idx == 300 and val == 0.0 and bool(np.signbit(val)) == (first < 0)


def test_assess_optim_zero_cut_and_infinite_margins(gpu):
    X, lab = clouds(999, 6, 1.0, 2)
    o = gpu.SvmOracle(X, lab)
    # an all-NaN x: every margin is NaN, nothing is below +inf -> (0, +inf), the zero cut, gamma = +0.0
    (g, cut), shrunk, gamma = o.assess_optim(np.full(7, np.nan), -5.0)
    assert shrunk and not g.any() and g.size == 7 and cut.beta == 0.0
    assert same_bits(gamma, 0.0) and o.last()[0] == 0 and o.last()[1] == np.inf
    # a separating point: min_val >= 1 -> the zero cut
    x = np.zeros(7)
    x[0] = 4.0
    (g, cut), _, gamma = o.assess_optim(x, 0.5)
    assert not g.any() and same_bits(gamma, 0.0) and o.last()[1] >= 1.0
    check_assess(o, X, lab, x)
    # a -inf margin (and a later one): the first wins, the gradient carries the infinity
    X2 = X.copy()
    X2[400, 0] = -np.inf
    X2[800, 0] = -np.inf
    lab2 = lab.copy()
    lab2[400] = lab2[800] = 1
    o2 = gpu.SvmOracle(X2, lab2)
    idx, val = check_assess(o2, X2, lab2, x)
    assert idx == 400 and val == -np.inf


# ---- the device loop against the host-driven loop: same handle type and depth, bit for bit ----------------------------

def host_loop(o, space, gamma, max_iters, tol):
    """cutting_plane_optim with the device oracle behind assess_optim and ellhip_update for the space"""
    x_best, chosen = None, []
    for niter in range(max_iters):
        cut, shrunk, gamma = o.assess_optim(space.xc(), gamma)
        chosen.append(o.last()[0])
        x_best = space.xc()
        status = space.update_central_cut(cut)
        if int(status) != 0 or space.tsq() < tol:
            return x_best, niter, gamma, chosen
    return x_best, max_iters, gamma, chosen


def new_space(gpu, variant, n, kappa, depth=None):
    if variant == "ell":
        s = gpu.Ell.new_with_scalar(kappa, np.zeros(n))
        if depth is not None:
            s.defer_depth = depth
        return s
    return gpu.EllStable.new_with_scalar(kappa, np.zeros(n))


def assert_same_state(a, b):
    assert same_bits(a.xc(), b.xc()) and same_bits(a.mq, b.mq)
    assert same_bits(a.kappa, b.kappa) and same_bits(a.tsq(), b.tsq())


LOOP_CASES = [  # name, (m, nfeat, shift), kappa, max_iters, tol
    ("separable", (1000, 7, 0.6), 10.0, 3000, 1e-14),     # ends on the zero cut (NaN state, tsq = 0 < tol)
    ("overlap", (777, 5, 0.1), 10.0, 3000, 1e-5),         # ends on tsq < tol
    ("max_iters", (4099, 63, 0.1), 10.0, 150, 1e-30),     # runs to max_iters
    ("tol0", (1000, 7, 0.6), 10.0, 120, 0.0),             # past the zero cut on a NaN state
]


@pytest.mark.parametrize("variant,depth", [("ell", 1), ("ell", 8), ("stable", None)])
@pytest.mark.parametrize("name,shape,kappa,max_iters,tol", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_device_loop_equals_host_loop(gpu, variant, depth, name, shape, kappa, max_iters, tol):
    X, lab = clouds(*shape, seed=1)
    o = gpu.SvmOracle(X, lab)
    n = shape[1] + 1
    sh = new_space(gpu, variant, n, kappa, depth)
    sd = new_space(gpu, variant, n, kappa, depth)
    xb_h, ni_h, gm_h, chosen = host_loop(o, sh, -1.0, max_iters, tol)
    xb_d, ni_d, gm_d = o.cutting_plane_optim(sd, -1.0, max_iters, tol)
    assert ni_d == ni_h and xb_d is not None
    assert same_bits(xb_d, xb_h) and same_bits(gm_d, gm_h)
    assert_same_state(sd, sh)
    # the oracle's last scan is the last iteration's
    assert o.last()[0] == chosen[-1]
    # the space stays usable: a second run continues from where the first left off, on both sides
    if name == "overlap":
        xb_h2, ni_h2, gm_h2, _ = host_loop(o, sh, gm_h, 7, 0.0)
        xb_d2, ni_d2, gm_d2 = o.cutting_plane_optim(sd, gm_d, 7, 0.0)
        assert ni_d2 == ni_h2 and same_bits(xb_d2, xb_h2) and same_bits(gm_d2, gm_h2)
        assert_same_state(sd, sh)


# ---- the device loop against the reference loop over the CPU oracle -----------------------------------------------

def oracle_space(orc, variant, n, kappa):
    cls = orc.OracleEll if variant == "ell" else orc.OracleEllStable
    return cls.new_with_scalar(kappa, np.zeros(n))


def assert_close_on_mask(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), what
    if (~na).any():
        assert rel_inf(a[~na], b[~nb]) <= TOL, (what, rel_inf(a[~na], b[~nb]))


@pytest.mark.parametrize("variant", ["ell", "stable"])
@pytest.mark.parametrize("name,shape,kappa,max_iters,tol", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_device_loop_matches_reference_loop(gpu, orc, variant, name, shape, kappa, max_iters, tol):
    X, lab = clouds(*shape, seed=1)
    n = shape[1] + 1
    es = oracle_space(orc, variant, n, kappa)
    xb_r, ni_r, gm_r, chosen_r = ref.cutting_plane_optim(X, lab, es, -1.0, max_iters, tol)
    o = gpu.SvmOracle(X, lab)
    _, ni_h, _, chosen_h = host_loop(o, new_space(gpu, variant, n, kappa), -1.0, max_iters, tol)
    assert ni_h == ni_r and chosen_h == chosen_r
    sd = new_space(gpu, variant, n, kappa)
    xb_d, ni_d, gm_d = o.cutting_plane_optim(sd, -1.0, max_iters, tol)
    assert ni_d == ni_r
    assert_close_on_mask(xb_d, xb_r, "x_best")
    assert_close_on_mask([gm_d], [gm_r], "gamma")
    assert_close_on_mask(sd.xc(), es.xc, "xc")
    assert_close_on_mask(sd.mq, es.mq, "Q")
    assert_close_on_mask([sd.kappa], [es.kappa], "kappa")
    assert_close_on_mask([sd.tsq()], [es.tsq], "tsq")
    if name == "separable":   # the zero cut ended it: gamma = +0.0 and the state is NaN
        assert same_bits(gm_d, 0.0) and np.isnan(sd.xc()).all() and sd.tsq() == 0.0


def test_device_loop_at_depth_24(gpu, orc):
    """n = 5120 (nfeat = 5119): a new Ell starts on the lower-triangle schedule at depth 24"""
    X, lab = clouds(1500, 5119, 0.3, seed=4)
    o = gpu.SvmOracle(X, lab)
    sd = gpu.Ell.new_with_scalar(10.0, np.zeros(5120))
    sh = gpu.Ell.new_with_scalar(10.0, np.zeros(5120))
    assert sd.defer_depth == 24
    xb_d, ni_d, gm_d = o.cutting_plane_optim(sd, -1.0, 12, 1e-30)
    xb_h, ni_h, gm_h, chosen_h = host_loop(o, sh, -1.0, 12, 1e-30)
    assert ni_d == ni_h == 12 and same_bits(xb_d, xb_h) and same_bits(gm_d, gm_h)
    assert_same_state(sd, sh)
    es = orc.OracleEll.new_with_scalar(10.0, np.zeros(5120))
    xb_r, ni_r, gm_r, chosen_r = ref.cutting_plane_optim(X, lab, es, -1.0, 12, 1e-30)
    assert ni_r == 12 and chosen_h == chosen_r
    assert rel_inf(xb_d, xb_r) <= TOL and abs(gm_d - gm_r) <= TOL * abs(gm_r)
    assert rel_inf(sd.xc(), es.xc) <= TOL and rel_inf(sd.mq, es.mq) <= TOL


# ---- through the C++ host mirror (ellalgo-rs_amd/host/ellhip/svm_hip.hpp) -------------------------------------------

def test_cpp_host_mirror_host_and_device_loops_agree(gpu):
    import cpp_build
    exe = cpp_build.build_runner("svm_runner.cpp", "hip")
    res = cpp_build.run_json_lines(exe)
    for case in ("separable_ell", "overlap_ell", "overlap_stable", "max_iters_ell"):
        h, d = res[case + "_host"], res[case + "_device"]
        assert h["niter"] == d["niter"] and h["has_x"] and d["has_x"], case
        assert h["x"] == d["x"] and h["gamma"] == d["gamma"] and h["tsq"] == d["tsq"], case
    assert res["max_iters_ell_device"]["niter"] == 150
    assert res["separable_ell_device"]["gamma"] == "0000000000000000"   # ended on the zero cut


# ---- invalid calls ------------------------------------------------------------------------------------------------

def test_invalid_calls(gpu):
    L = gpu.capi.load()
    X, lab = clouds(100, 7, 0.5, seed=9)
    o = gpu.SvmOracle(X, lab)
    gm, hb, ni = C.c_double(0.0), C.c_int(), C.c_int64()
    xb = np.empty(8)
    # n != nfeat + 1
    s = gpu.Ell.new_with_scalar(1.0, np.zeros(7))
    assert L.ellhip_svm_optim(s._h, o._h, C.byref(gm), 10, 1e-8, xb.ctypes.data, C.byref(hb), C.byref(ni)) == gpu.capi.E_INVALID
    with pytest.raises(gpu.capi.EllHipError):
        o.cutting_plane_optim(s, 0.0, 10, 1e-8)
    # a row shard
    h = C.c_void_p()
    gpu.capi.check(L.ellhip_create_shard(C.byref(h), 8, 0, 4, 1.0, None, None, None, -1))
    try:
        assert L.ellhip_svm_optim(h, o._h, C.byref(gm), 10, 1e-8, xb.ctypes.data, C.byref(hb), C.byref(ni)) == \
            gpu.capi.E_INVALID
    finally:
        L.ellhip_destroy(h)
    # m = 0
    assert L.ellhip_svm_create(C.byref(h), 0, 7, X.ctypes.data, lab.ctypes.data, -1) == gpu.capi.E_INVALID and not h.value
    # max_iters = 0: nothing runs, gamma untouched
    s = gpu.Ell.new_with_scalar(1.0, np.zeros(8))
    assert o.cutting_plane_optim(s, 0.25, 0, 1e-8) == (None, 0, 0.25)
