"""CPU: include/ellhip_batch_lowpass.h is valid C99, the binding lists exactly what it declares and libellhip.so exports
it, the kernels are part of the build recipe, the loop refuses to run without a HIP device (no CPU fallback), and the CPU
reference runs the GPU tests compare against (tests/batch_lowpass_reference.py) are pinned."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_lowpass_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_lowpass.h")
NAMES = ["ellhip_batch_lowpass_" + s for s in ("create", "destroy", "assess_feas", "assess_optim", "state", "reset",
                                                 "get_spectrum", "optim", "feas", "set_chunk")]


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_batch_lowpass_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_lowpass_h.c"
    src.write_text('#include "ellhip_batch_lowpass.h"\nint main(void) { ellhip_batch_lowpass *o = 0; '
                   'ellhip_batch_lowpass_destroy(o); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    assert declared_functions() == sorted(NAMES)
    assert declared_functions() == sorted(pkg.capi.BATCH_LOWPASS_EXPORTS)
    assert not set(pkg.capi.BATCH_LOWPASS_EXPORTS) & set(pkg.capi.EXPORTS + pkg.capi.SVM_EXPORTS + pkg.capi.BATCH_LMI_EXPORTS)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_kernels_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_lowpass_kernels.hpp" in pkg.build.HEADERS
    assert "batch_lowpass_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_lowpass.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_lowpass_capi.inc.hpp")).read()
    assert '#include "batch_lowpass_capi.inc.hpp"' in main and '#include "batch_lowpass_kernels.hpp"' in inc
    assert pkg.BatchLowpassProblem is not None


def test_invalid_shapes_and_no_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    h = C.c_void_p()

    def create(B, n, consts):
        cols = ref.columns(consts)
        return lib.ellhip_batch_lowpass_create(C.byref(h), B, n, *[c.ctypes.data for c in cols], None, -1)

    good = [ref.LOOSE, ref.CORRECTED]
    for B, n, consts in ((0, 8, good), (-1, 8, good), (2, 0, good), (2, 129, good),
                         (2, 8, [ref.LOOSE, (0.3, 0.2, 0.5, 1.5, 0.3)]),            # wpass > wstop
                         (2, 8, [ref.LOOSE, (-0.1, 0.2, 0.5, 1.5, 0.3)]),
                         (2, 8, [ref.LOOSE, (0.1, 1.2, 0.5, 1.5, 0.3)]),
                         (2, 8, [ref.LOOSE, (float("nan"), 0.2, 0.5, 1.5, 0.3)])):
        assert create(B, n, consts) == pkg.capi.E_INVALID and not h.value
        assert lib.ellhip_last_error()
    if lib.ellhip_device_count() > 0:  # (on a GPU machine: the same arguments create a handle)
        assert create(2, 8, good) == 0 and h.value
        lib.ellhip_batch_lowpass_destroy(h)
        return
    assert create(2, 8, good) == pkg.capi.E_NODEVICE and not h.value
    assert b"no HIP device" in lib.ellhip_last_error()
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchLowpassProblem(8, *ref.columns(good))


# ---- the CPU runs the GPU tests lean on (computed from the CPU oracle) ---------------------------------------------------
PINS = [
    ("corrected", 32, ref.CORRECTED, 12481, ref.SUCCESS, 0.0004135142518411313),
    ("corrected", 48, ref.CORRECTED, 6693, ref.SUCCESS, 4.354409725139092e-06),
    ("as written", 32, ref.AS_WRITTEN, 0, ref.NOSOLN, None),
    ("short passband", 32, ref.SHORT_PASSBAND, 969, ref.SUCCESS, 2.1710931196961606e-08),
    ("empty transition band", 16, ref.EMPTY_TRANSITION, 65, ref.NOSOLN, None),
    ("no stopband", 8, ref.NO_STOPBAND_A, 10, ref.UNKNOWN, None),
    ("no stopband", 8, ref.NO_STOPBAND_B, 10, ref.UNKNOWN, None),
]


@pytest.mark.parametrize("name,n,consts,niter,status,gamma", PINS, ids=[f"{p[0]}-{p[1]}-{p[2][0]}" for p in PINS])
def test_optim_pins(name, n, consts, niter, status, gamma):
    r = ref.solve_optim(n, consts)
    assert r["niter"] == niter and r["status"] == status
    if gamma is None:  # no best point, gamma unchanged
        assert r["x_best"] is None and r["gamma"] == consts[4]
    else:
        assert r["x_best"] is not None and r["gamma"] == gamma


def test_state_pins():
    s = ref.solve_optim(32, ref.CORRECTED)["state"]
    assert (s["idx1"], s["idx2"], s["idx3"], s["kmax"]) == (57, 95, 99, 97) and s["fmax"] == 0.0001198239990649856
    s = ref.solve_optim(32, ref.SHORT_PASSBAND)["state"]
    assert s["nwpass"] == 10 and s["nwpass"] < 32
    s = ref.solve_optim(16, ref.EMPTY_TRANSITION)["state"]
    assert s["nwpass"] == s["nwstop"]
    for c in (ref.NO_STOPBAND_A, ref.NO_STOPBAND_B):
        s = ref.solve_optim(8, c)["state"]
        assert s["nwstop"] == 15 * 8 and s["kmax"] == -1 and s["more_alt"] == 0


def test_feas_pins():
    r = ref.solve_feas(16, ref.LOOSE)
    assert r["x_best"] is not None and r["niter"] == 17 and r["status"] == ref.SUCCESS
    r = ref.solve_feas(32, ref.CORRECTED)
    assert r["x_best"] is not None and r["niter"] == 69 and r["status"] == ref.SUCCESS
    r = ref.solve_feas(32, ref.FEAS_INFEASIBLE)
    assert r["x_best"] is None and r["niter"] == 187 and r["status"] == ref.NOSOLN


@pytest.mark.parametrize("n,lo,hi", [(16, 3719, 4991), (32, 6433, 13233)])
def test_family_ends_with_a_best_point(n, lo, hi):
    runs = [ref.solve_optim(n, ref.family(s)) for s in range(6)]
    assert all(r["x_best"] is not None and r["niter"] < ref.MAX_ITERS and r["status"] == ref.SUCCESS for r in runs)
    niters = [r["niter"] for r in runs]
    assert min(niters) == lo and max(niters) == hi and len(set(niters)) == 6


def test_records_are_read_only():
    r = ref.solve_optim(32, ref.SHORT_PASSBAND)
    with pytest.raises(ValueError):
        r["xc"][0] = 1.0
