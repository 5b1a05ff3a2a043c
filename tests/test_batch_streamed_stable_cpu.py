"""CPU: include/ellhip_batch_streamed_stable.h is valid C99, the binding lists exactly what it declares and libellhip.so
exports it, the sources are part of the build recipe, the mirrors offer the constructors, without a device they refuse
loudly, and the engine's scratch-triangle map (csrc/batch_streamed_stable_layout.hpp) is a one-to-one map of the strict lower
triangle onto itself (a stand-alone host program under AddressSanitizer + UBSan)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cpp_build import CPP, OUT, _newer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_streamed_stable.h")
NAMES = ["ellhip_batch_create_streamed_stable", "ellhip_batch_streamed_stable_from_space"]


def declared_functions(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_streamed_stable_h.c"
    src.write_text('#include "ellhip_batch_streamed_stable.h"\n'
                   "int main(void) { int (*f)(ellhip_batch **, const ellhip_space *, int64_t) = "
                   "ellhip_batch_streamed_stable_from_space;\n"
                   "    int (*g)(ellhip_batch **, int64_t, int64_t, const double *, const double *, const double *, "
                   "const double *, int) = ellhip_batch_create_streamed_stable;\n"
                   "    return f == 0 || g == 0 || ELLHIP_BATCH_STREAMED_NMAX != 1024; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    assert declared_functions() == sorted(NAMES) == sorted(capi.BATCH_STREAMED_STABLE_EXPORTS)
    others = (capi.EXPORTS + capi.SVM_EXPORTS + capi.BATCH_LMI_EXPORTS + capi.BATCH_LOWPASS_EXPORTS + capi.BATCH_SVM_EXPORTS +
              capi.LMI_LOOP_EXPORTS + capi.BATCH_STABLE_LOOP_EXPORTS + capi.BATCH_STREAMED_EXPORTS +
              capi.BATCH_LOWPASS_STREAMED_EXPORTS)
    assert not set(NAMES) & set(others)
    # the streamed header keeps its three declarations and points at the new one
    streamed = os.path.join(ROOT, "include", "ellhip_batch_streamed.h")
    assert declared_functions(streamed) == sorted(capi.BATCH_STREAMED_EXPORTS) and len(capi.BATCH_STREAMED_EXPORTS) == 3
    text = open(streamed).read()
    assert "ellhip_batch_streamed_stable.h" in text and "Not offered: EllStable" not in text


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_sources_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    for name in ("batch_streamed_stable_kernels.hpp", "batch_streamed_stable_layout.hpp", "batch_streamed_stable_capi.inc.hpp"):
        assert name in pkg.build.HEADERS
    assert "ellhip_batch_streamed_stable.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    assert '#include "batch_streamed_stable_capi.inc.hpp"' in main
    assert main.index('#include "batch_streamed_capi.inc.hpp"') < main.index('#include "batch_streamed_stable_capi.inc.hpp"')
    layout = open(os.path.join(pkg.build.CSRC, "batch_streamed_stable_layout.hpp")).read()
    assert "hip/" not in layout   # the CPU program below builds it alone


def test_python_and_cpp_mirrors_offer_the_constructors(tmp_path):
    import ellalgo_rs_amd as pkg
    assert issubclass(pkg.EllStableBatchStreamed, pkg.EllStableBatch) and "EllStableBatchStreamed" in pkg.__all__
    assert not issubclass(pkg.EllStableBatchStreamed, pkg.EllBatch)
    assert pkg.EllStableBatchStreamed._create == "ellhip_batch_create_streamed_stable"
    assert pkg.EllStableBatchStreamed._from_space == "ellhip_batch_streamed_stable_from_space"
    assert isinstance(pkg.EllStableBatchStreamed.is_streamed, property)
    assert not hasattr(pkg.EllStableBatchStreamed, "set_no_defer_trick") and not hasattr(pkg.EllStableBatch, "is_streamed")
    host = os.path.join(pkg.build.HOST_DIR, "ellhip")
    src = tmp_path / "streamed_stable.cpp"
    src.write_text('#include "ell_batch_hip.hpp"\n'
                   "using namespace ellhip;\n"
                   "bool f(const Arr& k, const std::vector<Arr>& m, const std::vector<Arr>& x, EllStableHip& e, EllHip& l) {\n"
                   "    EllStableBatchStreamedHip a = EllStableBatchStreamedHip::new_with_scalar(k, x);\n"
                   "    EllStableBatchStreamedHip b = EllStableBatchStreamedHip::make(m, x);\n"
                   "    EllStableBatchStreamedHip c = EllStableBatchStreamedHip::new_with_matrix(k, m, x);\n"
                   "    EllStableBatchStreamedHip d = EllStableBatchStreamedHip::from_space(e, 4);\n"
                   "    EllBatchStreamedHip s = EllBatchStreamedHip::from_space(l, 4);\n"
                   "    d.set_use_parallel_cut(false);\n"
                   "    return a.is_streamed() && b.is_streamed() && c.is_streamed() && d.is_streamed() && s.is_streamed();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", host, str(src)])
    bad = tmp_path / "streamed_stable_no_defer.cpp"   # no_defer_trick exists on Ell only
    bad.write_text('#include "ell_batch_hip.hpp"\n'
                   "void f(ellhip::EllStableBatchStreamedHip& a) { a.set_no_defer_trick(true); }\n")
    assert subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", host, str(bad)], capture_output=True).returncode != 0


def test_no_device_means_loud_failure_not_fallback():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    if lib.ellhip_device_count() > 0:
        pytest.skip("a HIP device is visible here")
    h = C.c_void_p()
    assert lib.ellhip_batch_create_streamed_stable(C.byref(h), 4, 200, None, None, None, None, -1) == pkg.capi.E_NODEVICE
    assert not h.value and b"no HIP device" in lib.ellhip_last_error()
    assert lib.ellhip_batch_streamed_stable_from_space(C.byref(h), None, 4) == pkg.capi.E_NODEVICE
    with pytest.raises(pkg.capi.EllHipError):
        pkg.EllStableBatchStreamed.new_with_scalar(np.ones(4), np.zeros((4, 200)))


def test_scratch_map_is_one_to_one_onto_the_free_slots():
    """tests/cpp/streamed_stable_layout_check.cpp: n in {1, 2, 3, 64, 65, 1000, 1024}"""
    import ellalgo_rs_amd as pkg
    os.makedirs(OUT, exist_ok=True)
    header = os.path.join(pkg.build.CSRC, "batch_streamed_stable_layout.hpp")
    src, exe = os.path.join(CPP, "streamed_stable_layout_check.cpp"), os.path.join(OUT, "streamed_stable_layout_check")
    if _newer(exe, [src, header]):
        # (the sanitizer runtimes linked statically: the program needs nothing from its environment to start)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", pkg.build.CSRC,
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                               "-static-libubsan", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and r.stdout.strip().endswith("streamed_stable_layout_check: ok"), (r.returncode, r.stdout, r.stderr)
