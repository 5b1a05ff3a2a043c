"""CPU: the EllStable entry points of the batched engine (include/ellhip_batch.h) -- plain C99 declarations, exported
with the signatures the binding lists, and a loud ELLHIP_E_NODEVICE instead of a CPU path when no device is present."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ellhip_batch_create_stable", "ellhip_batch_stable_from_space", "ellhip_batch_variant")

C_USE = r"""
#include "ellhip_batch.h"
int use(ellhip_batch *h, const ellhip_space *s, const double *mq) {
    ellhip_batch *a = 0, *b = 0;
    int rc = ellhip_batch_create_stable(&a, 4, 3, 0, mq, 0, 0, -1);
    rc |= ellhip_batch_stable_from_space(&b, s, 8);
    return rc | ellhip_batch_variant(h) | (ellhip_batch_variant(a) == ELLHIP_SPACE_ELL_STABLE);
}
"""


def test_new_declarations_are_valid_c99(tmp_path):
    src = tmp_path / "use_batch_stable.c"
    src.write_text(C_USE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_new_symbols_are_declared_listed_and_exported():
    import ellalgo_rs_amd as pkg
    from test_capi_symbols import declared_functions
    lib = C.CDLL(pkg.capi.lib_path())
    for name in NEW:
        assert name in declared_functions() and name in pkg.capi.EXPORTS
        assert getattr(lib, name) is not None
    assert "batch_stable_kernels.hpp" in pkg.build.HEADERS


def test_new_entry_points_fail_loudly_without_a_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    if lib.ellhip_device_count() > 0:
        pytest.skip("a HIP device is visible here")
    h = C.c_void_p()
    assert lib.ellhip_batch_create_stable(C.byref(h), 4, 8, None, None, None, None, -1) == pkg.capi.E_NODEVICE
    assert not h.value and b"no HIP device" in lib.ellhip_last_error()
    assert lib.ellhip_batch_stable_from_space(C.byref(h), None, 4) == pkg.capi.E_NODEVICE
    assert not h.value and b"no HIP device" in lib.ellhip_last_error()
    assert lib.ellhip_batch_variant(None) == pkg.capi.E_NODEVICE
    for ctor in (lambda: pkg.EllStableBatch.new_with_scalar(np.ones(4), np.zeros((4, 8))),
                 lambda: pkg.EllStableBatch.new(np.ones((4, 8)), np.zeros((4, 8))),
                 lambda: pkg.EllStableBatch.new_with_matrix(1.0, np.zeros((4, 8, 8)), np.zeros((4, 8)))):
        with pytest.raises(pkg.capi.EllHipError):
            ctor()
