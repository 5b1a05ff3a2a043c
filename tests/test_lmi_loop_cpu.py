"""CPU: include/ellhip_lmi_loop.h is valid C99, the binding lists exactly what it declares and libellhip.so exports it, the
lists of entry points are disjoint, the kernels are part of the build recipe, and without a device the handle refuses loudly
(no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_lmi_loop.h")
NAMES = ["ellhip_lmi_loop_" + s for s in ("create", "destroy", "get_idx", "set_idx", "assess_optim", "assess_feas", "optim",
                                          "feas")]


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "lmi_loop_h.c"
    src.write_text('#include "ellhip_lmi_loop.h"\nint main(void) { ellhip_lmi_loop *o = 0; '
                   'ellhip_lmi_loop_destroy(o); return ELLHIP_LMI_LOOP_JMAX == 8 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    assert declared_functions() == sorted(NAMES)
    assert declared_functions() == sorted(pkg.capi.LMI_LOOP_EXPORTS)


def test_lists_are_disjoint():
    import ellalgo_rs_amd as pkg
    lists = [pkg.capi.EXPORTS, pkg.capi.SVM_EXPORTS, pkg.capi.BATCH_LMI_EXPORTS, pkg.capi.BATCH_LOWPASS_EXPORTS,
             pkg.capi.BATCH_SVM_EXPORTS, pkg.capi.LMI_LOOP_EXPORTS]
    names = [n for l in lists for n in l]
    assert len(names) == len(set(names))
    # ellhip_lmi.h keeps its own symbols only: the loop's live in their own header
    lmi_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ellhip_lmi.h")).read(), flags=re.S)
    assert "ellhip_lmi_loop" not in lmi_h


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_kernels_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "lmi_loop_kernels.hpp" in pkg.build.HEADERS
    assert "lmi_loop_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_lmi_loop.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "lmi_loop_capi.inc.hpp")).read()
    assert '#include "lmi_loop_capi.inc.hpp"' in main and '#include "lmi_loop_kernels.hpp"' in inc
    assert pkg.LmiLoopProblem is not None


def test_invalid_arguments_and_no_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    h = C.c_void_p(0xdead)
    blocks = (C.c_void_p * 9)()
    for J in (0, -1, 9):
        h.value = 0xdead
        assert lib.ellhip_lmi_loop_create(C.byref(h), C.cast(blocks, C.c_void_p), J, None) == pkg.capi.E_INVALID and not h.value
        assert lib.ellhip_last_error()
    assert lib.ellhip_lmi_loop_create(C.byref(h), None, 1, None) == pkg.capi.E_INVALID and not h.value
    assert lib.ellhip_lmi_loop_create(None, C.cast(blocks, C.c_void_p), 1, None) == pkg.capi.E_INVALID
    i = C.c_int()
    assert lib.ellhip_lmi_loop_get_idx(None, C.byref(i)) == pkg.capi.E_INVALID
    assert lib.ellhip_lmi_loop_set_idx(None, 0) == pkg.capi.E_INVALID
    lib.ellhip_lmi_loop_destroy(None)
    with pytest.raises(pkg.capi.EllHipError):
        pkg.LmiLoopProblem([])
    if lib.ellhip_device_count() > 0:  # (on a GPU machine a NULL block is what is wrong with this call)
        assert lib.ellhip_lmi_loop_create(C.byref(h), C.cast(blocks, C.c_void_p), 1, None) == pkg.capi.E_INVALID
        return
    h.value = 0xdead
    assert lib.ellhip_lmi_loop_create(C.byref(h), C.cast(blocks, C.c_void_p), 1, None) == pkg.capi.E_NODEVICE and not h.value
    assert b"no HIP device" in lib.ellhip_last_error()
    with pytest.raises(pkg.capi.EllHipError):   # the blocks themselves have no CPU path either
        pkg.LmiLoopProblem([pkg.LMIOracle(np.zeros((2, 3, 3)), np.eye(3))], c=np.ones(2))
