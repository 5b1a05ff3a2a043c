"""CPU: the SVM oracle's restatement reproduces the reference's unit tests, include/ellhip_svm.h is valid C99, the
binding lists exactly what the header declares and libellhip.so exports it, and the oracle refuses to run without a
HIP device (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import svm_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reference_unit_tests():
    # svm_oracle.rs:66-78 test_svm_oracle: improved
    data = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
    (g, beta), shrunk, gamma, idx, val = ref.assess_optim(data, [1, 1, -1, -1], np.zeros(3))
    assert shrunk
    assert idx == 0 and val == 0.0 and gamma == val == beta
    assert np.array_equal(g, [-0.0, -0.0, -1.0])
    # :80-90 test_svm_oracle_optimal: separable two-point case, gamma == 0.0
    (g, beta), shrunk, gamma, idx, val = ref.assess_optim(np.array([[1.0, 0.0], [-1.0, 0.0]]), [1, -1],
                                                          np.array([1.0, 0.0, 0.0]))
    assert shrunk and gamma == 0.0 and beta == 0.0 and val == 1.0
    assert np.signbit(gamma) == 0 and not g.any() and g.size == 3


def test_restatement_margin_fold_and_argmin_rule():
    # the fold starts at -0.0: with every product -0.0 and b = -0.0 the margin keeps the sign (a +0.0 start would not)
    mg = ref.margins(np.ones((2, 3)), [1, -1], np.full(4, -0.0))
    assert np.signbit(mg).tolist() == [True, False] and not mg.any()
    # left fold, not a pairwise sum: 1e16 + 1 + 1 stays 1e16 from the left
    mg = ref.margins(np.array([[1e16, 1.0, 1.0]]), [1], np.array([1.0, 1.0, 1.0, 0.0]))
    assert mg[0] == 1e16
    # ties go to the first index and keep its value; NaN never wins
    assert ref.argmin(np.array([np.nan, 0.0, -0.0, -1.0, -1.0])) == (3, -1.0)
    i, v = ref.argmin(np.array([0.0, -0.0]))
    assert i == 0 and not np.signbit(v)
    assert ref.argmin(np.array([np.nan, np.inf])) == (0, np.inf)


def svm_declared_functions():
    src = open(os.path.join(ROOT, "include", "ellhip_svm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_svm_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "svm_h.c"
    src.write_text('#include "ellhip_svm.h"\nint main(void) { ellhip_svm *o = 0; ellhip_svm_destroy(o); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    assert svm_declared_functions() == sorted(pkg.capi.SVM_EXPORTS)
    assert not set(pkg.capi.SVM_EXPORTS) & set(pkg.capi.EXPORTS)


@pytest.mark.parametrize("name", svm_declared_functions())
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_invalid_sizes_and_no_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    h = C.c_void_p()
    data = np.zeros(6)
    lab = np.ones(3, dtype=np.int32)
    for m, nfeat in ((0, 2), (3, 0), (-1, 2)):
        assert lib.ellhip_svm_create(C.byref(h), m, nfeat, data.ctypes.data, lab.ctypes.data, -1) == pkg.capi.E_INVALID
        assert not h.value
    if lib.ellhip_device_count() > 0:  # (on a GPU machine: the same arguments create an oracle)
        assert lib.ellhip_svm_create(C.byref(h), 3, 2, data.ctypes.data, lab.ctypes.data, -1) == 0 and h.value
        lib.ellhip_svm_destroy(h)
        return
    assert lib.ellhip_svm_create(C.byref(h), 3, 2, data.ctypes.data, lab.ctypes.data, -1) == pkg.capi.E_NODEVICE
    assert not h.value and b"no HIP device" in lib.ellhip_last_error()
    with pytest.raises(pkg.capi.EllHipError):
        pkg.SvmOracle(data.reshape(3, 2), [1, -1, 1])
