"""CPU: include/ellhip_batch_lowpass_streamed.h is valid C99, the binding lists exactly what it declares and libellhip.so
exports it, the sources are part of the build recipe, without a device the constructor refuses loudly, and the CPU reference
runs the GPU tests compare against (tests/batch_lowpass_reference.py, at the filter lengths past the LDS engine) are pinned,
so a drifting reference is noticed before a GPU is blamed."""
import ctypes as C
import os
import re
import subprocess

import pytest

import batch_lowpass_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_lowpass_streamed.h")
NAMES = ["ellhip_batch_lowpass_create_streamed", "ellhip_batch_lowpass_optim_streamed", "ellhip_batch_lowpass_feas_streamed"]


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_lowpass_streamed_h.c"
    src.write_text('#include "ellhip_batch_lowpass_streamed.h"\n'
                   "int main(void) { ellhip_batch_lowpass *o = 0; return ellhip_batch_lowpass_feas_streamed(0, o, 0, 0.0, 0, 0, 0, 0); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    assert declared_functions() == sorted(NAMES) == sorted(capi.BATCH_LOWPASS_STREAMED_EXPORTS)
    others = (capi.EXPORTS + capi.SVM_EXPORTS + capi.BATCH_LMI_EXPORTS + capi.BATCH_LOWPASS_EXPORTS + capi.BATCH_SVM_EXPORTS +
              capi.LMI_LOOP_EXPORTS + capi.BATCH_STABLE_LOOP_EXPORTS + capi.BATCH_STREAMED_EXPORTS)
    assert not set(NAMES) & set(others)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_sources_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_streamed_loop_kernels.hpp" in pkg.build.HEADERS
    assert "batch_lowpass_streamed_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_lowpass_streamed.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_loop_capi.inc.hpp")).read()
    assert '#include "batch_lowpass_streamed_capi.inc.hpp"' in main and '#include "batch_streamed_loop_kernels.hpp"' in inc
    assert callable(pkg.BatchLowpassProblem.streamed)


def test_cpp_mirror_offers_the_streamed_form(tmp_path):
    import ellalgo_rs_amd as pkg
    host = os.path.join(pkg.build.HOST_DIR, "ellhip")
    src = tmp_path / "streamed_lowpass.cpp"
    src.write_text('#include "batch_lowpass_hip.hpp"\n'
                   "using namespace ellhip;\n"
                   "std::size_t f(const std::vector<LowpassSpec>& specs, EllBatchStreamedHip& s, EllBatchHip& l, Arr& gamma) {\n"
                   "    BatchLowpassHip a = BatchLowpassHip::streamed(300, specs);\n"
                   "    BatchLowpassHip b(64, specs);\n"
                   "    return a.optim(s, gamma, Options(10, 1e-8)).niter[0] + a.feas(s, Options(10, 1e-8)).niter[0] +\n"
                   "           b.optim(l, gamma, Options(10, 1e-8)).niter[0];\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", host, str(src)])


def test_invalid_shapes_and_no_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    h = C.c_void_p()

    def create(B, n, consts):
        cols = ref.columns(consts)
        return lib.ellhip_batch_lowpass_create_streamed(C.byref(h), B, n, *[c.ctypes.data for c in cols], None, -1)

    good = [ref.LOOSE, ref.CORRECTED]
    for B, n, consts in ((0, 200, good), (2, 0, good), (2, 1025, good), (2, 200, [ref.LOOSE, (0.3, 0.2, 0.5, 1.5, 0.3)])):
        assert create(B, n, consts) == pkg.capi.E_INVALID and not h.value
        assert lib.ellhip_last_error()
    if lib.ellhip_device_count() > 0:  # (on a GPU machine: the same arguments create a handle)
        assert create(2, 200, good) == 0 and h.value
        lib.ellhip_batch_lowpass_destroy(h)
        return
    assert create(2, 200, good) == pkg.capi.E_NODEVICE and not h.value
    assert b"no HIP device" in lib.ellhip_last_error()
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchLowpassProblem.streamed(200, *ref.columns(good))
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchLowpassProblem(129, *ref.columns(good))  # the LDS engine's constructor keeps its limit


# ---- the CPU runs the GPU tests lean on (computed from the CPU oracle on OracleEll.new_with_scalar(40, 0), tolerance 1e-14) --
# n, constants, optim niter, optim status, optim has a best point, feas niter, feas finds a point
PINS = [
    (129, ref.LOOSE, 2252, ref.NOSOLN, True, 148, True),
    (130, ref.SHORT_PASSBAND, 2246, ref.NOSOLN, True, 142, True),
    (130, ref.EMPTY_TRANSITION, 337, ref.NOSOLN, False, 337, False),
    (129, ref.NO_STOPBAND_B, 212, ref.UNKNOWN, False, 212, True),
    (129, ref.NO_STOPBAND_A, 177, ref.UNKNOWN, False, 177, True),
    (130, ref.FEAS_INFEASIBLE, 846, ref.NOSOLN, True, 300, True),
    (191, ref.CORRECTED, 2641, ref.NOSOLN, True, 284, True),
    (200, ref.family(1), 3193, ref.NOSOLN, True, 250, True),
    (256, ref.LOOSE, 4275, ref.NOSOLN, True, 300, True),
]


@pytest.mark.parametrize("n,consts,niter,status,best,fniter,feasible", PINS, ids=[f"{p[0]}-{p[1][0]}-{p[1][1]}" for p in PINS])
def test_complete_run_pins(n, consts, niter, status, best, fniter, feasible):
    r = ref.solve_optim(n, consts)
    assert (r["niter"], r["status"], r["x_best"] is not None) == (niter, status, best)
    if not best:
        assert r["gamma"] == consts[4]
    f = ref.solve_feas(n, consts)
    assert (f["niter"], f["x_best"] is not None) == (fniter, feasible)
    assert f["status"] == (ref.SUCCESS if feasible else ref.NOSOLN)


def test_cut_off_pins():
    r = ref.solve_optim(512, ref.LOOSE, 700)
    assert r["niter"] == 700 and r["status"] == ref.SUCCESS and r["x_best"] is not None and r["gamma"] == 0.1536537185113417
    f = ref.solve_feas(512, ref.LOOSE)
    assert f["niter"] == 608 and f["x_best"] is not None
    for consts in (ref.LOOSE, ref.family(0)):
        r = ref.solve_optim(1024, consts, 150)
        assert r["niter"] == 150 and r["status"] == ref.SUCCESS and r["x_best"] is None
        f = ref.solve_feas(1024, consts, 150)
        assert f["niter"] == 150 and f["status"] == ref.SUCCESS and f["x_best"] is None


def test_the_mixed_batch_stops_at_different_iterations():
    runs = [ref.solve_optim(136, c) for c in [ref.family(s) for s in range(6)] + [ref.NO_STOPBAND_B, ref.EMPTY_TRANSITION]]
    assert len({r["niter"] for r in runs}) > 4
    assert runs[6]["status"] == ref.UNKNOWN and runs[6]["niter"] < min(r["niter"] for r in runs[:6])
