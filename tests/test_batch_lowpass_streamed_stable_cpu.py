"""CPU: include/ellhip_batch_lowpass_streamed_stable.h is valid C99, the binding lists exactly what it declares and
libellhip.so exports it, the sources are part of the build recipe, the mirrors pick the new entry points for a streamed
EllStable batch, without a device the entry points refuse loudly, the loop's LDS need stays within 64 KiB at every n the
streamed engine takes, and the CPU reference runs the GPU tests compare against (tests/batch_stable_loop_reference.py:
oracle.OracleLowpass over oracle.OracleEllStable) are pinned, so a drifting reference is noticed before a GPU is blamed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_lowpass_reference as lp
import batch_stable_loop_reference as ref
from cpp_build import CPP, OUT, _newer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_lowpass_streamed_stable.h")
NAMES = ["ellhip_batch_lowpass_optim_streamed_stable", "ellhip_batch_lowpass_feas_streamed_stable"]
UNCAPPED = lp.MAX_ITERS


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_lowpass_streamed_stable_h.c"
    src.write_text('#include "ellhip_batch_lowpass_streamed_stable.h"\n'
                   "int main(void) { ellhip_batch_lowpass *o = 0; double g = 0.0;\n"
                   "    return ellhip_batch_lowpass_feas_streamed_stable(0, o, 0, 0.0, 0, 0, 0, 0) +\n"
                   "           ellhip_batch_lowpass_optim_streamed_stable(0, o, &g, 0, 0.0, 0, 0, 0, 0); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    assert declared_functions() == sorted(NAMES) == sorted(capi.BATCH_LOWPASS_STREAMED_STABLE_EXPORTS)
    others = (capi.EXPORTS + capi.SVM_EXPORTS + capi.BATCH_LMI_EXPORTS + capi.BATCH_LOWPASS_EXPORTS + capi.BATCH_SVM_EXPORTS +
              capi.LMI_LOOP_EXPORTS + capi.BATCH_STABLE_LOOP_EXPORTS + capi.BATCH_STREAMED_EXPORTS +
              capi.BATCH_LOWPASS_STREAMED_EXPORTS + capi.BATCH_STREAMED_STABLE_EXPORTS)
    assert not set(NAMES) & set(others)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_sources_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_streamed_stable_loop_kernels.hpp" in pkg.build.HEADERS
    assert "batch_lowpass_streamed_stable_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_lowpass_streamed_stable.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_loop_capi.inc.hpp")).read()
    assert main.index('#include "batch_lowpass_capi.inc.hpp"') < main.index('#include "batch_lowpass_streamed_stable_capi.inc.hpp"')
    assert '#include "batch_streamed_stable_loop_kernels.hpp"' in inc
    kernels = open(os.path.join(pkg.build.CSRC, "batch_streamed_stable_loop_kernels.hpp")).read()
    assert "bs_stable_cut(" in kernels and '#include "batch_streamed_stable_kernels.hpp"' in kernels


def test_python_mirror_picks_the_entry_point_by_handle():
    import ellalgo_rs_amd as pkg
    from ellalgo_rs_amd.batch_lowpass import _loop_entry

    class Handle:
        def __init__(self, variant, streamed):
            self.variant = variant
            if streamed is not None:
                self.is_streamed = streamed

    ell, stable = pkg.capi.SPACE_ELL, pkg.capi.SPACE_ELL_STABLE
    for name in ("ellhip_batch_lowpass_optim", "ellhip_batch_lowpass_feas"):
        assert _loop_entry(Handle(ell, None), name) == name
        assert _loop_entry(Handle(stable, None), name) == name + "_stable"
        assert _loop_entry(Handle(ell, True), name) == name + "_streamed"
        assert _loop_entry(Handle(stable, True), name) == name + "_streamed_stable"
        assert name + "_streamed_stable" in pkg.capi.BATCH_LOWPASS_STREAMED_STABLE_EXPORTS


def test_cpp_mirror_offers_the_streamed_stable_form(tmp_path):
    import ellalgo_rs_amd as pkg
    host = os.path.join(pkg.build.HOST_DIR, "ellhip")
    src = tmp_path / "streamed_stable_lowpass.cpp"
    src.write_text('#include "batch_lowpass_hip.hpp"\n'
                   "using namespace ellhip;\n"
                   "std::size_t f(const std::vector<LowpassSpec>& specs, EllStableBatchStreamedHip& s, EllBatchStreamedHip& e,\n"
                   "              EllStableBatchHip& l, Arr& gamma) {\n"
                   "    BatchLowpassHip a = BatchLowpassHip::streamed(300, specs);\n"
                   "    return a.optim(s, gamma, Options(10, 1e-8)).niter[0] + a.feas(s, Options(10, 1e-8)).niter[0] +\n"
                   "           a.optim(e, gamma, Options(10, 1e-8)).niter[0] + a.feas(l, Options(10, 1e-8)).niter[0];\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", host, str(src)])
    mirror = open(os.path.join(host, "batch_lowpass_hip.hpp")).read()
    for name in NAMES:
        assert name in mirror


def test_no_device_or_no_handle_means_a_refusal_not_a_fallback():
    """without a device no handle can be made, so the entry points can only be reached with NULL handles: a refusal with a
    message, never a result, and the outputs stay as the caller left them"""
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    gamma = np.full(2, 0.3)
    x = np.full((2, 129), np.nan)
    has = np.full(2, 7, dtype=np.int32)
    niter = np.full(2, 7, dtype=np.int64)
    status = np.full(2, 7, dtype=np.int32)
    refusals = (pkg.capi.E_NODEVICE, pkg.capi.E_INVALID)
    assert lib.ellhip_batch_lowpass_optim_streamed_stable(None, None, p(gamma), 10, 1e-8, p(x), p(has), p(niter), p(status)) in refusals
    assert lib.ellhip_last_error()
    assert lib.ellhip_batch_lowpass_feas_streamed_stable(None, None, 10, 1e-8, p(x), p(has), p(niter), p(status)) in refusals
    assert lib.ellhip_last_error()
    assert np.isnan(x).all() and (gamma == 0.3).all() and (has == 7).all() and (niter == 7).all() and (status == 7).all()
    if lib.ellhip_device_count() > 0:
        return
    with pytest.raises(pkg.capi.EllHipError):   # neither half of the pair can be made here
        pkg.EllStableBatchStreamed.new_with_scalar(np.full(2, lp.KAPPA), np.zeros((2, 129)))
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchLowpassProblem.streamed(129, *lp.columns([lp.LOOSE] * 2))


def test_lds_need_stays_within_64_kib():
    """tests/cpp/streamed_stable_loop_lds_check.hip: batch_streamed_stable_loop_lds_doubles<BatchLpOracle> at every
    1 <= n <= 1024, on the host"""
    import ellalgo_rs_amd as pkg
    os.makedirs(OUT, exist_ok=True)
    src, exe = os.path.join(CPP, "streamed_stable_loop_lds_check.hip"), os.path.join(OUT, "streamed_stable_loop_lds_check")
    deps = [src] + [os.path.join(pkg.build.CSRC, f) for f in pkg.build.HEADERS]
    if _newer(exe, deps):
        subprocess.check_call([pkg.build._hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall",
                               "-Werror", "-Wno-unused-function", "-I", pkg.build.CSRC, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("streamed_stable_loop_lds_check: ok"), (r.returncode, r.stdout, r.stderr)
    at_1024 = int(re.search(r"bytes at n = 1024: (\d+)", r.stdout).group(1))
    assert at_1024 == 8 * (4 * 1024 + 72 + 1045) <= 64 * 1024


# ---- the CPU runs the GPU tests lean on: EllStable::new_with_scalar(lp.KAPPA, 0), tol = lp.TOL ------------------------------
def run(n, consts, *, feas=False, max_iters=UNCAPPED):
    return ref.cpu_run(ref.lp_case(n, [consts], feas=feas, max_iters=max_iters))[0]


# n, constants, optim (niter, status), feas (niter, feasible)
COMPLETE = [
    (129, lp.EMPTY_TRANSITION, (1203, ref.NOSOLN), (1203, False)),
    (129, lp.NO_STOPBAND_B, (724, ref.UNKNOWN), (724, True)),
    (130, lp.NO_STOPBAND_B, (732, ref.UNKNOWN), (732, True)),
    (130, lp.EMPTY_TRANSITION, (1220, ref.NOSOLN), (1220, False)),
] + [(130, lp.family(s), (k, ref.NOSOLN), (k, False)) for s, k in enumerate((143, 154, 165, 179, 196, 217))]


@pytest.mark.parametrize("n,consts,optim,feas", COMPLETE, ids=[f"{c[0]}-{c[1][0]:.2f}-{c[1][1]:.2f}" for c in COMPLETE])
def test_complete_run_pins(n, consts, optim, feas):
    r = run(n, consts)
    assert (r["niter"], r["status"]) == optim and r["x_best"] is None and r["gamma"] == consts[4]
    f = run(n, consts, feas=True)
    assert (f["niter"], f["x_best"] is not None) == feas
    assert f["status"] == (ref.SUCCESS if feas[1] else ref.NOSOLN)


def test_loose_pins():
    r = run(129, lp.LOOSE, max_iters=1500)   # (the uncapped run goes on for more than 6000 rounds)
    assert (r["niter"], r["status"]) == (1500, ref.SUCCESS) and r["x_best"] is not None and r["gamma"] < 0.3
    f = run(129, lp.LOOSE, feas=True)
    assert (f["niter"], f["status"]) == (728, ref.SUCCESS) and f["x_best"] is not None


@pytest.mark.parametrize("n,max_iters", [(512, 150), (1023, 40), (1024, 60), (193, 300)])
def test_cut_off_pins(n, max_iters):
    r = run(n, lp.LOOSE, max_iters=max_iters)
    assert (r["niter"], r["status"]) == (max_iters, ref.SUCCESS) and r["x_best"] is None


def test_the_mixed_batch_stops_at_eight_different_rounds():
    consts = [lp.family(s) for s in range(6)] + [lp.NO_STOPBAND_B, lp.EMPTY_TRANSITION]
    runs = ref.cpu_run(ref.lp_case(130, consts, max_iters=UNCAPPED))
    assert len({r["niter"] for r in runs}) == 8 and len({r["status"] for r in runs}) == 2
    feas = ref.cpu_run(ref.lp_case(130, consts, feas=True, max_iters=UNCAPPED))
    assert {(r["status"], r["x_best"] is not None) for r in feas} == {(ref.NOSOLN, False), (ref.SUCCESS, True)}
    assert [r["niter"] for r in feas] == [r["niter"] for r in runs]
