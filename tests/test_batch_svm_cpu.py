"""CPU: include/ellhip_batch_svm.h is valid C99, the binding lists exactly what it declares and libellhip.so exports it,
the kernels are part of the build recipe, the entry points refuse bad shapes before they look for a device and refuse to
run without one (no CPU fallback), and the CPU reference runs the GPU tests compare against
(tests/batch_svm_reference.py) are pinned."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_svm_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_svm.h")
NAMES = ["ellhip_batch_svm_" + s for s in ("create", "destroy", "margins", "assess_optim", "last", "optim", "set_chunk")]


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_batch_svm_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_svm_h.c"
    src.write_text('#include "ellhip_batch_svm.h"\nint main(void) { ellhip_batch_svm *o = 0; '
                   'ellhip_batch_svm_destroy(o); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    assert declared_functions() == sorted(NAMES)
    assert declared_functions() == sorted(pkg.capi.BATCH_SVM_EXPORTS)
    others = pkg.capi.EXPORTS + pkg.capi.SVM_EXPORTS + pkg.capi.BATCH_LMI_EXPORTS + pkg.capi.BATCH_LOWPASS_EXPORTS
    assert not set(pkg.capi.BATCH_SVM_EXPORTS) & set(others)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_kernels_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_svm_kernels.hpp" in pkg.build.HEADERS
    assert "batch_svm_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_svm.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_svm_capi.inc.hpp")).read()
    assert '#include "batch_svm_capi.inc.hpp"' in main and '#include "batch_svm_kernels.hpp"' in inc
    assert pkg.BatchSvmProblem is not None


def test_invalid_shapes_and_no_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    h = C.c_void_p()
    data = np.zeros((2, 4, 128))
    lab = np.ones((2, 4), dtype=np.int32)

    def create(B, m, nfeat, d=data, l=lab, shared=0):
        return lib.ellhip_batch_svm_create(C.byref(h), B, m, nfeat, None if d is None else d.ctypes.data, shared,
                                           None if l is None else l.ctypes.data, -1)

    for args in ((0, 4, 3), (-1, 4, 3), ((1 << 24) + 1, 4, 3), (2, 0, 3), (2, (1 << 24) + 1, 3), (2, 4, 0), (2, 4, 128),
                 (2, 4, 3, None, lab), (2, 4, 3, data, None), (2, 4, 3, None, lab, 1)):
        h.value = 0xdead
        assert create(*args) == pkg.capi.E_INVALID and not h.value, args
        assert lib.ellhip_last_error()
    if lib.ellhip_device_count() > 0:  # (on a GPU machine: the same arguments create a handle)
        for nfeat, shared in ((3, 0), (127, 0), (3, 1)):
            assert create(2, 4, nfeat, shared=shared) == 0 and h.value
            lib.ellhip_batch_svm_destroy(h)
        return
    for nfeat, shared in ((3, 0), (127, 0), (3, 1)):
        assert create(2, 4, nfeat, shared=shared) == pkg.capi.E_NODEVICE and not h.value
        assert b"no HIP device" in lib.ellhip_last_error()
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchSvmProblem(data[:, :, :3], lab)
    with pytest.raises(ValueError):
        pkg.BatchSvmProblem(data[0], lab[0])      # labels must be B x m
    with pytest.raises(ValueError):
        pkg.BatchSvmProblem(data[:, :3], lab)     # m differs


# ---- the CPU runs the GPU tests lean on (svm_reference over the CPU oracle) ----------------------------------------------
@pytest.mark.parametrize("m,nfeat,tol,max_iters,niters", ref.ROWS, ids=[f"{r[0]}x{r[1]}" for r in ref.ROWS])
def test_family_pins(m, nfeat, tol, max_iters, niters):
    runs = [ref.solve(s, m, nfeat, max_iters, tol) for s in range(6)]
    assert tuple(r["niter"] for r in runs) == niters
    for s, r in enumerate(runs):
        assert r["status"] == ref.SUCCESS and r["x_best"] is not None
        if s % 3 == 0:  # separable: the reference's zero cut ends it, and leaves a NaN space
            assert r["gamma"] == 0.0 and not np.signbit(r["gamma"]) and r["tsq"] == 0.0 and np.isnan(r["xc"]).all()
            assert r["min_val"] >= 1.0
        elif s % 3 == 1 and r["niter"] < max_iters:  # shift 0.2: the tolerance, with a negative gamma
            assert r["gamma"] < 0.0 and r["tsq"] < tol and r["gamma"] == r["min_val"]
        if r["niter"] == max_iters:
            assert r["tsq"] >= tol


def test_tol_zero_runs_past_the_zero_cut():
    X, lab = ref.family(0, 64, 2)
    r = ref.run(X, lab, 10, 0.0)
    assert r["niter"] == 10 and r["gamma"] == 0.0 and np.isnan(r["xc"]).all() and np.isnan(r["tsq"])
    assert (r["min_idx"], r["min_val"]) == (0, np.inf) and r["status"] == ref.SUCCESS


def test_max_iters_zero_keeps_everything():
    X, lab = ref.family(1, 64, 2)
    r = ref.run(X, lab, 0, 1e-8, gamma=-3.0, last=(5, 0.25))
    assert r["x_best"] is None and r["niter"] == 0 and r["gamma"] == -3.0 and (r["min_idx"], r["min_val"]) == (5, 0.25)
    assert r["kappa"] == ref.KAPPA and not r["xc"].any()


def test_records_are_read_only():
    r = ref.solve(3, 64, 2, 2000, 1e-12)
    with pytest.raises(ValueError):
        r["xc"][0] = 1.0
    with pytest.raises(ValueError):
        r["x_best"][0] = 1.0
