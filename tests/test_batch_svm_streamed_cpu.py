"""CPU: include/ellhip_batch_svm_streamed.h is valid C99, the binding lists exactly what it declares and libellhip.so exports
it, the sources are part of the build recipe, the mirrors pick the new entry points for streamed batches, the constructor
refuses nfeat = 0 and nfeat = 1024 before it looks for a device and answers E_NODEVICE without one, the two loops' LDS needs
follow the header's formulas and stay within 64 KiB at every n, and the CPU reference runs the GPU tests compare against
(tests/batch_svm_reference.py over oracle.OracleEll, tests/batch_stable_loop_reference.py over oracle.OracleEllStable) are
pinned, so a drifting reference is noticed before a GPU is blamed.  `ell_record` and `stable_record` cache those runs for
tests/test_gpu_batch_svm_streamed.py."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import batch_stable_loop_reference as sref
import batch_svm_reference as ref
from cpp_build import CPP, OUT, _newer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_svm_streamed.h")
NAMES = ["ellhip_batch_svm_create_streamed", "ellhip_batch_svm_optim_streamed", "ellhip_batch_svm_optim_streamed_stable"]
TOL = 1e-12
INF = np.inf

# (m, nfeat, s), max_iters; Ell: niter, zero cut?, gamma or None, min_idx or None; EllStable: the same four
PINS = [
    ((40, 128, 0), 400, (53, True, None, None), (53, True, None, None)),
    ((200, 129, 0), 400, (100, True, None, 39), (98, True, None, 26)),
    ((70, 191, 3), 400, (93, True, None, None), (91, True, None, 65)),
    ((300, 256, 0), 400, (244, True, None, None), (244, True, None, 141)),
    ((24, 511, 0), 400, (136, True, None, None), (136, True, None, 1)),
    ((8, 1023, 0), 300, (84, True, None, 2), (82, True, None, 7)),
    ((16, 1023, 0), 300, (160, True, None, None), (159, True, None, 4)),
    ((200, 129, 1), 40, (40, False, -0.1141758457940361, None), (40, False, -0.11304030801134259, 40)),
    ((64, 1023, 0), 60, (60, False, 0.08468882884495597, None), (60, False, 0.08467672941491813, 28)),
    ((1100, 1023, 1), 8, (8, False, -0.018979681104154742, 1055), (8, False, -0.0189739193087649, 1055)),
]
PIN_IDS = ["%dx%d-s%d" % p[0] for p in PINS]
# six members of the family at (96, 128) whose runs end at six different rounds
MIXED = (96, 128, (0, 2, 3, 5, 6, 8), 400)
MIXED_NITER = (86, 306, 91, 298, 83, 332)


def ell_record(s, m, nfeat, max_iters, tol=TOL):
    """member s of the family on Ell::new_with_scalar(100, 0), gamma = +inf (cached and read-only in the reference module)"""
    return ref.solve(s, m, nfeat, max_iters, tol)


@functools.lru_cache(maxsize=None)
def stable_record(s, m, nfeat, max_iters, tol=TOL):
    """the same member on EllStable::new_with_scalar(100, 0), with min_idx / min_val beside the rest as in the Ell records"""
    case = sref.Case("svm", [ref.family(s, m, nfeat)], nfeat + 1, ref.KAPPA, np.zeros(nfeat + 1), max_iters=max_iters, tol=tol)
    r = sref.cpu_run(case)[0]
    r.update(r.pop("state"))
    return ref._freeze(r)


def record(stable, s, m, nfeat, max_iters, tol=TOL):
    return (stable_record if stable else ell_record)(s, m, nfeat, max_iters, tol)


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_svm_streamed_h.c"
    src.write_text('#include "ellhip_batch_svm_streamed.h"\n'
                   "int main(void) { ellhip_batch_svm *o = 0; double g = 0.0;\n"
                   "    return ellhip_batch_svm_create_streamed(&o, 1, 1, 1, 0, 0, 0, -1) +\n"
                   "           ellhip_batch_svm_optim_streamed(0, o, &g, 0, 0.0, 0, 0, 0, 0) +\n"
                   "           ellhip_batch_svm_optim_streamed_stable(0, o, &g, 0, 0.0, 0, 0, 0, 0) +\n"
                   "           ELLHIP_BATCH_STREAMED_NMAX; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])
    text = open(HEADER).read()
    for sibling in ("ellhip_batch_svm.h", "ellhip_batch_streamed.h", "ellhip_batch_streamed_stable.h"):
        assert f'#include "{sibling}"' in text


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    assert declared_functions() == sorted(NAMES) == sorted(capi.BATCH_SVM_STREAMED_EXPORTS)
    others = (capi.EXPORTS + capi.SVM_EXPORTS + capi.BATCH_LMI_EXPORTS + capi.BATCH_LOWPASS_EXPORTS + capi.BATCH_SVM_EXPORTS +
              capi.LMI_LOOP_EXPORTS + capi.BATCH_STABLE_LOOP_EXPORTS + capi.BATCH_STREAMED_EXPORTS +
              capi.BATCH_LOWPASS_STREAMED_EXPORTS + capi.BATCH_STREAMED_STABLE_EXPORTS +
              capi.BATCH_LOWPASS_STREAMED_STABLE_EXPORTS)
    assert not set(NAMES) & set(others)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_sources_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_svm_streamed_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_svm_streamed.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    new = main.index('#include "batch_svm_streamed_capi.inc.hpp"')
    for dep in ("batch_svm_capi.inc.hpp", "batch_loop_capi.inc.hpp"):
        assert main.index(f'#include "{dep}"') < new
    inc = open(os.path.join(pkg.build.CSRC, "batch_svm_streamed_capi.inc.hpp")).read()
    assert "batch_svm_run(" in inc and "BATCH_ENGINE_STREAMED)" in inc and "BATCH_ENGINE_STREAMED_STABLE)" in inc
    assert "batch_loop_run<BatchSvmOracle>" in open(os.path.join(pkg.build.CSRC, "batch_svm_capi.inc.hpp")).read()
    driver = open(os.path.join(pkg.build.CSRC, "batch_loop_capi.inc.hpp")).read()
    assert "k_batch_streamed_loop<Oracle>" in driver and "k_batch_streamed_loop_stable<Oracle>" in driver


def test_python_mirror_picks_the_entry_point_by_handle():
    import ellalgo_rs_amd as pkg
    from ellalgo_rs_amd.batch_svm import _loop_entry

    class Handle:
        def __init__(self, variant, streamed):
            self.variant = variant
            if streamed is not None:
                self.is_streamed = streamed

    ell, stable = pkg.capi.SPACE_ELL, pkg.capi.SPACE_ELL_STABLE
    name = "ellhip_batch_svm_optim"
    assert _loop_entry(Handle(ell, None), name) == name
    assert _loop_entry(Handle(stable, None), name) == name + "_stable"
    assert _loop_entry(Handle(ell, True), name) == name + "_streamed"
    assert _loop_entry(Handle(stable, True), name) == name + "_streamed_stable"
    assert callable(pkg.BatchSvmProblem.streamed)


def test_cpp_mirror_offers_the_streamed_form(tmp_path):
    import ellalgo_rs_amd as pkg
    host = os.path.join(pkg.build.HOST_DIR, "ellhip")
    src = tmp_path / "streamed_svm.cpp"
    src.write_text('#include "batch_svm_hip.hpp"\n'
                   "using namespace ellhip;\n"
                   "std::size_t f(const Arr& data, const std::vector<int32_t>& lab, EllStableBatchStreamedHip& s,\n"
                   "              EllBatchStreamedHip& e, EllStableBatchHip& l, EllBatchHip& q, Arr& gamma) {\n"
                   "    BatchSvmHip a = BatchSvmHip::streamed(2, 50, 300, data, true, lab);\n"
                   "    BatchSvmHip b(2, 50, 100, data, true, lab);\n"
                   "    return a.optim(s, gamma, Options(10, 1e-8)).niter[0] + a.optim(e, gamma, Options(10, 1e-8)).niter[0] +\n"
                   "           b.optim(l, gamma, Options(10, 1e-8)).niter[0] + b.optim(q, gamma, Options(10, 1e-8)).niter[0];\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", host, str(src)])
    mirror = open(os.path.join(host, "batch_svm_hip.hpp")).read()
    for name in NAMES:
        assert name in mirror


def test_create_refuses_before_it_looks_for_a_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    lab = np.ones((2, 4), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def create(nfeat, data=True, labels=True, B=2, m=4):
        h = C.c_void_p(12345)
        d = np.zeros((m, max(nfeat, 1)))
        rc = lib.ellhip_batch_svm_create_streamed(C.byref(h), B, m, nfeat, p(d) if data else None, 1, p(lab) if labels else None, -1)
        assert rc < 0 and h.value is None and lib.ellhip_last_error()
        return rc, lib.ellhip_last_error().decode()

    for nfeat in (0, 1024, -3):
        rc, msg = create(nfeat)
        assert rc == pkg.capi.E_INVALID and "1023" in msg
    assert create(5, data=False)[0] == pkg.capi.E_INVALID
    assert create(5, labels=False)[0] == pkg.capi.E_INVALID
    assert create(5, B=0)[0] == pkg.capi.E_INVALID
    assert create(5, m=0)[0] == pkg.capi.E_INVALID
    # the LDS engine's constructor keeps its own bound
    h = C.c_void_p()
    assert lib.ellhip_batch_svm_create(C.byref(h), 2, 4, 128, p(np.zeros((4, 128))), 1, p(lab), -1) == pkg.capi.E_INVALID
    assert "127" in lib.ellhip_last_error().decode()
    if lib.ellhip_device_count() > 0:
        return
    for nfeat in (1, 127, 128, 1023):
        assert create(nfeat)[0] == pkg.capi.E_NODEVICE
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchSvmProblem.streamed(np.zeros((4, 200)), lab)


def test_no_handle_means_a_refusal_not_a_fallback():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    gamma = np.full(2, 0.3)
    x = np.full((2, 129), np.nan)
    has = np.full(2, 7, dtype=np.int32)
    niter = np.full(2, 7, dtype=np.int64)
    status = np.full(2, 7, dtype=np.int32)
    for name in NAMES[1:]:
        assert getattr(lib, name)(None, None, p(gamma), 10, 1e-8, p(x), p(has), p(niter), p(status)) == pkg.capi.E_INVALID
        assert lib.ellhip_last_error()
    assert np.isnan(x).all() and (gamma == 0.3).all() and (has == 7).all() and (niter == 7).all() and (status == 7).all()


def test_lds_needs_follow_the_header_and_stay_within_64_kib():
    """tests/cpp/svm_streamed_loop_lds_check.hip: both loops' layout functions at every 1 <= n <= 1024, on the host"""
    import ellalgo_rs_amd as pkg
    os.makedirs(OUT, exist_ok=True)
    src, exe = os.path.join(CPP, "svm_streamed_loop_lds_check.hip"), os.path.join(OUT, "svm_streamed_loop_lds_check")
    deps = [src] + [os.path.join(pkg.build.CSRC, f) for f in pkg.build.HEADERS]
    if _newer(exe, deps):
        subprocess.check_call([pkg.build._hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall",
                               "-Werror", "-Wno-unused-function", "-I", pkg.build.CSRC, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("svm_streamed_loop_lds_check: ok"), (r.returncode, r.stdout, r.stderr)
    ell, stable = map(int, re.search(r"bytes at n = 1024: (\d+) \(Ell\) (\d+) \(EllStable\)", r.stdout).groups())
    assert ell == 8 * (5 * 1024 + 8 + 1035) <= 64 * 1024 and stable == 8 * (4 * 1024 + 72 + 1035) <= 64 * 1024
    header = open(HEADER).read()
    assert "48.1 KiB" in header and "40.6 KiB" in header
    assert round(ell / 1024, 1) == 48.1 and round(stable / 1024, 1) == 40.6


# ---- the CPU runs the GPU tests lean on -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,max_iters,ell,stable", PINS, ids=PIN_IDS)
def test_reference_pins(shape, max_iters, ell, stable):
    m, nfeat, s = shape
    for is_stable, (niter, zero, gamma, min_idx) in ((False, ell), (True, stable)):
        r = record(is_stable, s, m, nfeat, max_iters)
        assert r["niter"] == niter and r["status"] == ref.SUCCESS and r["x_best"] is not None, (is_stable, r["niter"])
        if zero:   # the zero cut: gamma = +0.0, tsq = 0.0 and the space NaN
            assert r["niter"] < max_iters and r["gamma"] == 0.0 and not np.signbit(r["gamma"]) and r["min_val"] >= 1.0
            assert np.isnan(r["xc"]).all() and r["tsq"] == 0.0
        else:
            assert r["niter"] == max_iters and r["gamma"] == gamma == r["min_val"] and np.isfinite(r["xc"]).all()
        if min_idx is not None:
            assert r["min_idx"] == min_idx, (is_stable, r["min_idx"])
    if shape == (40, 128, 0):
        assert np.isnan(record(False, s, m, nfeat, max_iters)["mq"]).all()


def test_the_mixed_batch_stops_at_six_different_rounds():
    m, nfeat, members, max_iters = MIXED
    assert tuple(ell_record(s, m, nfeat, max_iters)["niter"] for s in members) == MIXED_NITER
    assert len(set(MIXED_NITER)) == 6 and max(MIXED_NITER) < max_iters
    assert len({stable_record(s, m, nfeat, max_iters)["niter"] for s in members}) > 3


def test_tol_zero_runs_past_the_zero_cut_on_the_cpu():
    for stable in (False, True):
        assert record(stable, 0, 40, 128, 400)["niter"] == 53
        r = record(stable, 0, 40, 128, 59, 0.0)   # 53 rounds, the zero cut, 5 rounds on a NaN space
        assert r["niter"] == 59 and (r["min_idx"], r["min_val"]) == (0, INF) and np.isnan(r["xc"]).all()
        assert r["gamma"] == 0.0 and r["status"] == ref.SUCCESS
