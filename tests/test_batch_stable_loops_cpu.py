"""CPU: include/ellhip_batch_stable_loops.h is valid C99, the binding lists exactly what it declares and libellhip.so
exports it, the lists of entry points are disjoint, the three Ell headers keep what they declared, the new sources are
part of the build recipe, and without a device (or with NULL handles) the entry points refuse loudly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_stable_loops.h")
NAMES = ["ellhip_batch_lmi_optim_stable", "ellhip_batch_lmi_feas_stable", "ellhip_batch_lowpass_optim_stable",
         "ellhip_batch_lowpass_feas_stable", "ellhip_batch_svm_optim_stable"]


def declared_functions(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_stable_loops_h.c"
    src.write_text('#include "ellhip_batch_stable_loops.h"\n'
                   'int main(void) { int (*f)(ellhip_batch *, ellhip_batch_svm *, double *, int64_t, double, double *, '
                   'int32_t *, int64_t *, int32_t *) = ellhip_batch_svm_optim_stable; return f == 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    assert declared_functions() == sorted(NAMES)
    assert declared_functions() == sorted(pkg.capi.BATCH_STABLE_LOOP_EXPORTS)


def test_lists_are_disjoint_and_the_ell_headers_keep_their_own():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    lists = [capi.EXPORTS, capi.SVM_EXPORTS, capi.BATCH_LMI_EXPORTS, capi.BATCH_LOWPASS_EXPORTS, capi.BATCH_SVM_EXPORTS,
             capi.LMI_LOOP_EXPORTS, capi.BATCH_STABLE_LOOP_EXPORTS]
    names = [n for l in lists for n in l]
    assert len(names) == len(set(names))
    for header, own in (("ellhip_batch_lmi.h", capi.BATCH_LMI_EXPORTS), ("ellhip_batch_lowpass.h", capi.BATCH_LOWPASS_EXPORTS),
                        ("ellhip_batch_svm.h", capi.BATCH_SVM_EXPORTS)):
        path = os.path.join(ROOT, "include", header)
        assert declared_functions(path) == sorted(own)
        assert "ellhip_batch_stable_loops.h" in open(path).read()  # the comment that names where EllStable handles go
    assert len(capi.BATCH_LMI_EXPORTS) == 8


def test_signatures_equal_the_ell_counterparts():
    """each _stable prototype is its Ell counterpart's, in the header and in the binding"""
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()

    def proto(path, name):
        src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        return re.sub(r"\s+", " ", m.group(1)).replace(" *", "*").strip()

    for name in NAMES:
        base = name[:-len("_stable")]
        header = "ellhip_batch_" + base.split("_")[2] + ".h"
        assert proto(HEADER, name) == proto(os.path.join(ROOT, "include", header), base), name
        assert getattr(lib, name).argtypes == getattr(lib, base).argtypes
        assert getattr(lib, name).restype == getattr(lib, base).restype


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_sources_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_stable_apply.hpp" in pkg.build.HEADERS
    assert "batch_stable_loops_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_stable_loops.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    assert '#include "batch_stable_loops_capi.inc.hpp"' in main
    # the three oracles reach the EllStable cut through the one loop kernel they are policies of
    assert "batch_loop_kernels.hpp" in pkg.build.HEADERS and "batch_loop_capi.inc.hpp" in pkg.build.HEADERS
    assert '#include "batch_stable_apply.hpp"' in open(os.path.join(pkg.build.CSRC, "batch_loop_kernels.hpp")).read()
    for kernels in ("batch_lmi_kernels.hpp", "batch_lowpass_kernels.hpp", "batch_svm_kernels.hpp"):
        assert '#include "batch_loop_kernels.hpp"' in open(os.path.join(pkg.build.CSRC, kernels)).read()


def test_lds_formula_of_the_header():
    """s(n) of the header against the n = 128 figures it quotes: 128 * 129 + 3 * 128 + 8 is even, so | 1 adds one"""
    s = lambda n: (n * (n | 1) + 3 * n + 8) | 1
    assert s(128) == 16905 and s(1) == 13 and s(64) == 4361
    assert 8 * (s(128) + ((2 * 128 + 8 * 9 + 8 + 16) | 1)) <= 159 * 1024 < 8 * (s(128) + ((2 * 128 + 64 * 65 + 64 + 16) | 1))


def test_null_arguments_are_refused():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    out = np.zeros(4)
    p = out.ctypes.data_as(C.c_void_p)
    for name in NAMES:
        args = [None, None] + ([p] if "optim" in name else []) + [10, 1e-8, p, p, p, p]
        assert getattr(lib, name)(*args) == pkg.capi.E_INVALID, name
        assert lib.ellhip_last_error()


def test_host_mirror_dispatches_on_the_batch_variant(tmp_path):
    """host/ellhip/batch_{lmi,lowpass,svm}_hip.hpp: optim / feas compile for EllBatchHip and for EllStableBatchHip and
    name the entry point of the variant"""
    import ellalgo_rs_amd as pkg
    host = os.path.join(pkg.build.HOST_DIR, "ellhip")
    src = tmp_path / "dispatch.cpp"
    src.write_text('#include "batch_lmi_hip.hpp"\n#include "batch_lowpass_hip.hpp"\n#include "batch_svm_hip.hpp"\n'
                   "using namespace ellhip;\n"
                   "void f(BatchLmiHip& l, BatchLowpassHip& p, BatchSvmHip& s, EllBatchHip& e, EllStableBatchHip& t, Arr& g,\n"
                   "       const Options& o) {\n"
                   "    l.optim(e, g, o); l.optim(t, g, o); l.feas(e, o); l.feas(t, o);\n"
                   "    p.optim(e, g, o); p.optim(t, g, o); p.feas(e, o); p.feas(t, o);\n"
                   "    s.optim(e, g, o); s.optim(t, g, o);\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", host, str(src)])
    for name in ("batch_lmi_hip.hpp", "batch_lowpass_hip.hpp", "batch_svm_hip.hpp"):
        text = open(os.path.join(host, name)).read()
        stem = name[len("batch_"):-len("_hip.hpp")]
        assert f"ellhip_batch_{stem}_optim_stable" in text and "loop_entry(spaces, " in text
    assert "ELLHIP_SPACE_ELL_STABLE" in open(os.path.join(host, "ell_batch_hip.hpp")).read().split("loop_entry(const BatchHip")[1]
