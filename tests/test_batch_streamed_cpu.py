"""CPU: include/ellhip_batch_streamed.h is valid C99, the binding lists exactly what it declares and libellhip.so exports
it, the sources are part of the build recipe, and without a device the constructors refuse loudly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_streamed.h")
NAMES = ["ellhip_batch_create_streamed", "ellhip_batch_streamed_from_space", "ellhip_batch_is_streamed"]


def declared_functions(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_streamed_h.c"
    src.write_text('#include "ellhip_batch_streamed.h"\n'
                   "int main(void) { int (*f)(ellhip_batch **, const ellhip_space *, int64_t) = "
                   "ellhip_batch_streamed_from_space; return f == 0 || ELLHIP_BATCH_STREAMED_NMAX != 1024; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    assert declared_functions() == sorted(NAMES) == sorted(capi.BATCH_STREAMED_EXPORTS)
    others = (capi.EXPORTS + capi.SVM_EXPORTS + capi.BATCH_LMI_EXPORTS + capi.BATCH_LOWPASS_EXPORTS + capi.BATCH_SVM_EXPORTS +
              capi.LMI_LOOP_EXPORTS + capi.BATCH_STABLE_LOOP_EXPORTS)
    assert not set(NAMES) & set(others)
    assert capi.BATCH_STREAMED_NMAX == 1024
    assert "#define ELLHIP_BATCH_NMAX 128" in open(os.path.join(ROOT, "include", "ellhip_batch.h")).read()


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_sources_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_streamed_kernels.hpp" in pkg.build.HEADERS
    assert "batch_streamed_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_streamed.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    assert '#include "batch_streamed_capi.inc.hpp"' in main


def test_python_and_cpp_mirrors_offer_the_constructors(tmp_path):
    import ellalgo_rs_amd as pkg
    assert issubclass(pkg.EllBatchStreamed, pkg.EllBatch) and "EllBatchStreamed" in pkg.__all__
    assert pkg.EllBatchStreamed._create == "ellhip_batch_create_streamed"
    assert pkg.EllBatchStreamed._from_space == "ellhip_batch_streamed_from_space"
    assert pkg.EllBatch._create == "ellhip_batch_create" and not hasattr(pkg.EllBatch, "is_streamed")
    host = os.path.join(pkg.build.HOST_DIR, "ellhip")
    src = tmp_path / "streamed.cpp"
    src.write_text('#include "ell_batch_hip.hpp"\n'
                   "using namespace ellhip;\n"
                   "bool f(const Arr& k, const std::vector<Arr>& m, const std::vector<Arr>& x, EllHip& e) {\n"
                   "    EllBatchStreamedHip a = EllBatchStreamedHip::new_with_scalar(k, x);\n"
                   "    EllBatchStreamedHip b = EllBatchStreamedHip::make(m, x);\n"
                   "    EllBatchStreamedHip c = EllBatchStreamedHip::new_with_matrix(k, m, x);\n"
                   "    EllBatchStreamedHip d = EllBatchStreamedHip::from_space(e, 4);\n"
                   "    d.set_no_defer_trick(true);\n"
                   "    return a.is_streamed() && b.is_streamed() && c.is_streamed() && d.is_streamed();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", host, str(src)])


def test_no_device_means_loud_failure_not_fallback():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    if lib.ellhip_device_count() > 0:
        pytest.skip("a HIP device is visible here")
    h = C.c_void_p()
    assert lib.ellhip_batch_create_streamed(C.byref(h), 4, 200, None, None, None, None, -1) == pkg.capi.E_NODEVICE
    assert not h.value and b"no HIP device" in lib.ellhip_last_error()
    assert lib.ellhip_batch_streamed_from_space(C.byref(h), None, 4) == pkg.capi.E_NODEVICE
    assert lib.ellhip_batch_is_streamed(None) == pkg.capi.E_NODEVICE
    with pytest.raises(pkg.capi.EllHipError):
        pkg.EllBatchStreamed.new_with_scalar(np.ones(4), np.zeros((4, 200)))
