"""CPU: include/ellhip_batch_lmi.h is valid C99, the binding lists exactly what it declares and libellhip.so exports it,
the kernels are part of the build recipe, the loop refuses to run without a HIP device (no CPU fallback), and the CPU
restatement the GPU tests compare against (tests/batch_lmi_reference.py) is pinned on the reference problem."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_lmi_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "ellhip_batch_lmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_batch_lmi_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_lmi_h.c"
    src.write_text('#include "ellhip_batch_lmi.h"\nint main(void) { ellhip_batch_lmi *o = 0; ellhip_batch_lmi_destroy(o); '
                   'return ELLHIP_BATCH_LMI_JMAX + ELLHIP_BATCH_LMI_MMAX == 72 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    assert len(declared_functions()) == 8
    assert declared_functions() == sorted(pkg.capi.BATCH_LMI_EXPORTS)
    assert not set(pkg.capi.BATCH_LMI_EXPORTS) & set(pkg.capi.EXPORTS + pkg.capi.SVM_EXPORTS)


@pytest.mark.parametrize("name", declared_functions())
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_kernels_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_lmi_kernels.hpp" in pkg.build.HEADERS
    assert "batch_lmi_capi.inc.hpp" in pkg.build.HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_lmi_capi.inc.hpp")).read()
    assert '#include "batch_lmi_capi.inc.hpp"' in main and '#include "batch_lmi_kernels.hpp"' in inc


def test_invalid_shapes_and_no_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    fs, bs, c = ref.reference_problem()
    mat_f, mat_b, cc = ref.stack([(fs, bs, c)] * 2)
    flat_f = np.concatenate([f.ravel() for f in mat_f])
    flat_b = np.concatenate([b.ravel() for b in mat_b])
    h = C.c_void_p()

    def create(J, m):
        m = np.array(m, dtype=np.int64)
        return lib.ellhip_batch_lmi_create(C.byref(h), 2, 3, J, m.ctypes.data, flat_f.ctypes.data, flat_b.ctypes.data,
                                           cc.ctypes.data, -1)

    for J, m in ((0, [2, 3]), (9, [2] * 9), (2, [2, 65]), (2, [0, 3])):
        assert create(J, m) == pkg.capi.E_INVALID and not h.value
    if lib.ellhip_device_count() > 0:  # (on a GPU machine: the same arguments create a handle)
        assert create(2, [2, 3]) == 0 and h.value
        lib.ellhip_batch_lmi_destroy(h)
        return
    assert create(2, [2, 3]) == pkg.capi.E_NODEVICE and not h.value
    assert b"no HIP device" in lib.ellhip_last_error()
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchLmiProblem(mat_f, mat_b, cc)


def test_reference_problem_pin():
    """F1/B1, F2/B2 of tests/lmi_tests.rs:14-52 with c = (1, -1, 1) on Ell::new_with_scalar(10, 0), Options::default():
    the restatement stops where the CPU oracle's J = 2 restatement stops today (consistent with the reference's own
    `< 300`)."""
    fs, bs, c = ref.reference_problem()
    space = ref.new_space(3)
    omega = ref.RoundRobinLmi(fs, bs, c)
    x_best, niter, gamma, status = ref.optim(space, omega, math.inf, 2000, 1e-20)
    assert niter == 11 and status == ref.NOSOLN
    assert x_best is not None and gamma == -3.7502205782089257
    assert omega.idx in (0, 1, 2)


def test_round_robin_is_my_lmi_oracle_for_two_blocks():
    """call by call against a literal J = 2 walk (tests/lmi_tests.rs:145-171)"""
    fs, bs, c = ref.reference_problem()
    omega = ref.RoundRobinLmi(fs, bs, c)
    lmi = [ref.O.OracleLMI(fs[0], bs[0]), ref.O.OracleLMI(fs[1], bs[1])]
    idx, gamma_a, gamma_b = -1, math.inf, math.inf
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(60):
        x = rng.standard_normal(3) * rng.choice([0.1, 1.0, 3.0])
        (g, beta), station, gamma_a = omega.assess_optim(x, gamma_a)
        f0 = 0.0
        for a, b in zip(c.tolist(), x.tolist()):
            f0 += a * b
        want = None
        for _ in range(3):
            idx = 0 if idx == 2 else idx + 1
            if idx < 2:
                cut = lmi[idx].assess_feas(x)
                if cut is not None:
                    want = (cut[0], cut[1], idx)
                    break
            else:
                fj = f0 - gamma_b
                if fj > 0.0:
                    want = (c, fj, 2)
                    break
                gamma_b = f0
        if want is None:
            want = (c, 0.0, 3)
        assert station == want[2] and beta == want[1] and np.array_equal(g, want[0])
        assert omega.idx == idx and gamma_a == gamma_b
        seen.add(station)
    assert seen == {0, 1, 2, 3}


def test_families_stop_before_max_iters_with_a_best_point():
    runs, _, _ = ref.run_optim([ref.family_a(s) for s in range(8)], 2000, 1e-20)
    assert all(r["x_best"] is not None and r["niter"] < 2000 for r in runs)
    assert len({r["niter"] for r in runs}) >= 1
    runs, _, _ = ref.run_optim([ref.family_b(s, 8, 6, 2) for s in range(4)], 2000, 1e-10)
    assert all(r["x_best"] is not None and r["niter"] < 2000 and r["status"] == ref.SUCCESS for r in runs)
