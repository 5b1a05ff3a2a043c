"""CPU: csrc/ell_math.hpp compiled by plain g++ (tests/cpp/ell_math_host.cpp) equals its Python restatement bit for bit and is
within 1 ulp of mpmath; the reference's three pinned profit runs (83, 90, 29) with ell_exp / ell_log and with libm; the
conditions the GPU tests rely on in the seeded family (tests/batch_profit_reference.py); include/ellhip_batch_profit.h is
valid C99, the binding lists exactly what it declares and libellhip.so exports it; bad arguments are refused before a device
is looked for."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_profit_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_profit.h")
NAMES = ["ellhip_batch_profit_" + s for s in ("create", "destroy", "set_chunk", "assess_optim", "assess_optim_q", "optim",
                                              "optim_stable", "optim_q", "optim_q_stable")] + ["ellhip_math_eval"]
LOOPS = [n for n in NAMES if "_optim" in n and "assess" not in n]
FNS = ("exp", "log")


host_eval = ref.host_eval


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)   # a NaN is compared by position
    return a.shape == b.shape and bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


# ---- ell_exp / ell_log --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FNS)
def test_host_header_equals_the_restatement(fn):
    xs = ref.math_sweep(fn)
    assert xs.size >= 100_000
    f = ref.ell_exp if fn == "exp" else ref.ell_log
    want = np.array([f(float(x)) for x in xs])
    got = host_eval(fn, xs)
    assert same_bits(got, want), np.nonzero(got.view(np.int64) != want.view(np.int64))[0][:10]


def test_special_values():
    inf, nan = math.inf, math.nan
    e, l = ref.ell_exp, ref.ell_log
    assert e(inf) == inf and e(-inf) == 0.0 and not math.copysign(1.0, e(-inf)) < 0 and math.isnan(e(nan))
    assert e(0.0) == 1.0 and e(-0.0) == 1.0
    assert e(709.782712893384) == 1.7976931348622732e+308 and e(709.7827128933841) == inf and e(1e308) == inf
    assert e(-708.5) == 2.006132305331306e-308 and e(-744.0) == 1e-323                    # gradual underflow
    assert e(-745.1332191019411) == 5e-324 and e(-745.1332191019412) == 0.0 and e(-1e308) == 0.0
    assert l(0.0) == -inf and l(-0.0) == -inf and math.isnan(l(-1.0)) and math.isnan(l(-inf)) and math.isnan(l(-5e-324))
    assert l(inf) == inf and math.isnan(l(nan)) and l(1.0) == 0.0 and not math.copysign(1.0, l(1.0)) < 0
    assert l(5e-324) == math.log(5e-324) and l(1e-310) == math.log(1e-310)              # subnormal arguments
    assert l(2.2250738585072014e-308) == math.log(2.2250738585072014e-308)
    for x in ref.EXP_SPECIALS:
        assert same_bits(host_eval("exp", [x]), [e(x)]), x
    for x in ref.LOG_SPECIALS:
        assert same_bits(host_eval("log", [x]), [l(x)]), x


@pytest.mark.parametrize("fn", FNS)
def test_accuracy_against_mpmath(fn):
    """at most 1 ulp (the bound glibc documents for both), an ulp being that of the exact value's binade, 2^-1074 below
    2^-1022.  Worst found over this sweep: 0.718 ulp (exp, in the subnormal results; 0.612 over the normal results) and 0.772 ulp (log)."""
    import mpmath
    mpmath.mp.prec = 200
    xs = ref.math_sweep(fn)
    got = host_eval(fn, xs)
    exact_fn = mpmath.exp if fn == "exp" else mpmath.log
    worst, where = 0.0, None
    for x, g in zip(xs.tolist(), got.tolist()):
        if math.isnan(x) or math.isinf(x) or (fn == "log" and x <= 0.0):
            continue
        exact = exact_fn(mpmath.mpf(x))
        if exact == 0:
            assert g == 0.0
            continue
        if exact > mpmath.mpf(2) ** 1024:
            assert g == math.inf, x
            continue
        expo = max(int(mpmath.floor(mpmath.log(abs(exact), 2))), -1022)
        err = float(abs(mpmath.mpf(g) - exact) / mpmath.mpf(2) ** (expo - 52)) if not math.isinf(g) else math.inf
        if err > worst:
            worst, where = err, x
    print(f"ell_{fn}: worst error {worst:.4f} ulp at {where!r}")
    assert worst <= 1.0, (worst, where)


def test_round_is_half_away_from_zero():
    r = ref.rust_round
    assert [r(v) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 0.49999999999999994, 2.4999999999999996, 4503599627370497.0)] == \
        [1.0, 2.0, 3.0, -1.0, -3.0, 0.0, 2.0, 4503599627370497.0]
    assert r(math.inf) == math.inf and math.isnan(r(math.nan))


# ---- the reference's pins -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.KINDS))
def test_pins_with_both_arithmetics(name):
    kind = ref.KINDS[name]
    ours, libm = ref.pin_run(kind, ref.ELL), ref.pin_run(kind, ref.LIBM)
    for r in (ours, libm):
        assert r["niter"] == ref.PINS[kind] and r["x_best"] is not None
        assert r["x_best"][0] <= math.log(30.5)                              # src/oracles/profit_oracle.rs:185, :204, :222
    assert abs(ours["gamma"] - libm["gamma"]) <= 1e-6 * abs(libm["gamma"])   # the eps of the reference's assert_approx_eq
    assert np.all(np.abs(ours["x_best"] - libm["x_best"]) <= 1e-6 * np.abs(libm["x_best"]))


def test_reference_direct_call():
    """src/oracles/profit_oracle.rs:228-242"""
    for fns in (ref.ELL, ref.LIBM):
        omega = ref.ProfitOracle(ref.PIN_PARAMS, ref.PIN_A, ref.PIN_V, fns)
        (g, beta), feasible, gamma = omega.assess_optim([3.5, 2.0], 0.0)
        assert not feasible and beta == 3.5 - fns[1](30.5) and g == [1.0, 0.0]
        (g, beta), feasible, gamma = omega.assess_optim([3.0, 2.0], gamma)
        assert feasible and beta == 0.0 and gamma > 0.0


# ---- the family the GPU tests lean on -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", [False, True], ids=["ell", "stable"])
def test_family_conditions(stable):
    B = ref.FAMILY_B
    assert B == 200
    for kind in (ref.PLAIN, ref.ROBUST):
        runs = [ref.solve(kind, b, stable) for b in range(B)]
        assert all(r["x_best"] is not None for r in runs)
        assert all(r["status"] == ref.SUCCESS and 40 <= r["niter"] < ref.MAX_ITERS for r in runs)   # all end at the tolerance
        assert len({r["niter"] for r in runs}) > 10
    runs = [ref.solve(ref.DISCRETE, b, stable) for b in range(B)]
    assert sum(r["retries"] > 0 for r in runs) >= 2
    assert sum(r["status"] == ref.NOEFFECT for r in runs) >= 2
    assert sum(r["status"] == ref.NOSOLN for r in runs) >= 100
    assert all(r["x_best"] is not None and r["niter"] < ref.MAX_ITERS for r in runs)


def test_records_are_read_only():
    r = ref.solve(ref.PLAIN, 3)
    with pytest.raises(ValueError):
        r["xc"][0] = 1.0
    with pytest.raises(ValueError):
        r["x_best"][0] = 1.0


# ---- the surface --------------------------------------------------------------------------------------------------------------
def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_profit_h.c"
    src.write_text('#include "ellhip_batch_profit.h"\nint main(void) { ellhip_batch_profit *o = 0; '
                   'ellhip_batch_profit_destroy(o); return ELLHIP_PROFIT_PLAIN; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_ell_math_header_compiles_with_plain_gxx(tmp_path):
    src = tmp_path / "ell_math_h.cpp"
    src.write_text('#include "ell_math.hpp"\nint main() { return ellhip::ell_exp(0.0) == 1.0 && ellhip::ell_log(1.0) == 0.0 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "ellalgo-rs_amd", "csrc"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    assert declared_functions() == sorted(NAMES)
    assert declared_functions() == sorted(capi.BATCH_PROFIT_EXPORTS)
    others = [name for key, names in vars(capi).items() if key.endswith("EXPORTS") and key != "BATCH_PROFIT_EXPORTS"
              for name in names]
    assert len(others) > 150 and not set(capi.BATCH_PROFIT_EXPORTS) & set(others)
    assert (capi.PROFIT_PLAIN, capi.PROFIT_ROBUST, capi.PROFIT_DISCRETE) == (ref.PLAIN, ref.ROBUST, ref.DISCRETE)
    header = open(HEADER).read()
    for name, value in (("PLAIN", 0), ("ROBUST", 1), ("DISCRETE", 2)):
        assert f"#define ELLHIP_PROFIT_{name} {value}\n" in header


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_kernels_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    for f in ("ell_math.hpp", "batch_profit_kernels.hpp", "batch_profit_capi.inc.hpp"):
        assert f in pkg.build.HEADERS
    assert "ellhip_batch_profit.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_profit_capi.inc.hpp")).read()
    assert main.index('#include "batch_loop_capi.inc.hpp"') < main.index('#include "batch_profit_capi.inc.hpp"')
    assert '#include "batch_profit_kernels.hpp"' in inc and "batch_loop_drive" not in inc   # no second driver
    math_h = re.sub(r"//.*", "", open(os.path.join(pkg.build.CSRC, "ell_math.hpp")).read())
    assert not re.search(r"\b(fma|exp|log|ldexp|frexp|scalbn)\s*\(", math_h)                 # its own arithmetic only
    assert pkg.BatchProfitProblem is not None


def test_invalid_arguments_and_no_device():
    import ellalgo_rs_amd as pkg
    lib, E = pkg.capi.load(), pkg.capi.E_INVALID
    h = C.c_void_p()
    params, a, v, vp = np.full((2, 3), 20.0), np.full((2, 2), 0.2), np.full((2, 2), 10.0), np.full((2, 5), 0.5)
    p = lambda arr: None if arr is None else arr.ctypes.data_as(C.c_void_p)

    def create(B, kind, params=params, a=a, v=v, vp=None):
        return lib.ellhip_batch_profit_create(C.byref(h), B, kind, p(params), p(a), p(v), p(vp), -1)

    bad = [dict(B=0, kind=0), dict(B=-1, kind=0), dict(B=(1 << 24) + 1, kind=0), dict(B=2, kind=3), dict(B=2, kind=-1),
           dict(B=2, kind=0, params=None), dict(B=2, kind=0, a=None), dict(B=2, kind=0, v=None),
           dict(B=2, kind=1), dict(B=2, kind=0, vp=vp), dict(B=2, kind=2, vp=vp)]
    for args in bad:
        h.value = 0xdead
        assert create(**args) == E and not h.value, args
        assert lib.ellhip_last_error()
    assert lib.ellhip_batch_profit_create(None, 2, 0, p(params), p(a), p(v), None, -1) == E
    x, gamma, grad = np.zeros((2, 2)), np.zeros(2), np.zeros((2, 2))
    retry = np.zeros(2, dtype=np.int32)
    assert lib.ellhip_batch_profit_set_chunk(None, 8) == E
    assert lib.ellhip_batch_profit_assess_optim(None, p(x), p(gamma), p(grad), None, None) == E
    assert lib.ellhip_batch_profit_assess_optim_q(None, p(x), p(gamma), p(retry), p(grad), None, None, None, None) == E
    has, niter, status = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int64), np.full(2, 7, dtype=np.int32)
    xb = np.full((2, 2), np.nan)
    gamma[:] = 0.3
    for name in LOOPS:
        assert getattr(lib, name)(None, None, p(gamma), 10, 1e-8, p(xb), p(has), p(niter), p(status)) == E
        assert lib.ellhip_last_error()
    assert np.isnan(xb).all() and (gamma == 0.3).all() and (has == 7).all() and (niter == 7).all() and (status == 7).all()
    out = np.zeros(2)
    assert lib.ellhip_math_eval(2, 2, p(x), p(out), -1) == E and lib.ellhip_math_eval(0, 2, None, p(out), -1) == E
    assert lib.ellhip_math_eval(0, -1, p(x), p(out), -1) == E
    lib.ellhip_batch_profit_destroy(None)
    if lib.ellhip_device_count() > 0:   # (on a GPU machine: the same arguments create a handle)
        for kind, vpar in ((0, None), (1, vp), (2, None)):
            assert create(2, kind, vp=vpar) == 0 and h.value
            assert lib.ellhip_batch_profit_set_chunk(h, 0) == E and lib.ellhip_batch_profit_set_chunk(h, 4097) == E
            assert lib.ellhip_batch_profit_set_chunk(h, 4096) == 0
            lib.ellhip_batch_profit_destroy(h)
        return
    for kind, vpar in ((0, None), (1, vp), (2, None)):
        h.value = 0xdead
        assert create(2, kind, vp=vpar) == pkg.capi.E_NODEVICE and not h.value
        assert b"no HIP device" in lib.ellhip_last_error()
    assert lib.ellhip_math_eval(0, 2, p(x), p(out), -1) == pkg.capi.E_NODEVICE
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchProfitProblem("plain", params, a, v)
    with pytest.raises(ValueError):
        pkg.BatchProfitProblem("plain", params[:, :2], a, v)
    with pytest.raises(ValueError):
        pkg.BatchProfitProblem("plain", params, a[:1], v)
