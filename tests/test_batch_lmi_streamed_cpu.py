"""CPU: include/ellhip_batch_lmi_streamed.h is valid C99, the binding lists exactly what it declares and libellhip.so exports
it, the sources are part of the build recipe, the mirrors pick the new entry points for streamed batches, the constructor
refuses n = 0 and n = 1025 (and every bad shape) before it looks for a device and answers E_NODEVICE without one, the two
loops' LDS needs follow the header's formulas, and the CPU reference runs the GPU tests compare against
(tests/batch_lmi_streamed_cases.py: tests/batch_lmi_reference.py over oracle.OracleEll / OracleEllStable) are pinned, so a
drifting reference is noticed before a GPU is blamed.  The pinned set is also checked for what it covers -- every station
kind, failing pivot rows at both ends and between, every way a loop can end -- so the GPU comparisons cannot pass vacuously."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_lmi_streamed_cases as cases
from cpp_build import CPP, OUT, _newer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_lmi_streamed.h")
NAMES = ["ellhip_batch_lmi_create_streamed", "ellhip_batch_lmi_optim_streamed", "ellhip_batch_lmi_feas_streamed",
         "ellhip_batch_lmi_optim_streamed_stable", "ellhip_batch_lmi_feas_streamed_stable"]
SUCCESS, NOSOLN = 0, 1

# (batch, EllStable?, feas?) -> per member (niter, status, has a point, idx afterwards)
PINS = {
    ('129-64x3', False, False): [(30, 0, True, 2), (30, 0, True, 2), (30, 0, True, 1), (30, 0, True, 2), (30, 0, False, 2), (30, 0, True, 1)],
    ('129-64x3', False, True): [(0, 0, True, 1), (0, 0, True, 1), (1, 0, True, 1), (12, 0, True, 0), (30, 0, False, 0), (16, 0, True, 1)],
    ('129-64x3', True, False): [(30, 0, True, 2), (30, 0, True, 0), (30, 0, True, 1), (30, 0, True, 2), (30, 0, False, 2), (30, 0, True, 1)],
    ('129-64x3', True, True): [(0, 0, True, 1), (0, 0, True, 1), (1, 0, True, 1), (12, 0, True, 0), (30, 0, False, 0), (12, 0, True, 1)],
    ('130-64', False, False): [(30, 0, True, 1), (30, 0, True, 0), (30, 0, True, 1), (30, 0, False, 0), (30, 0, False, 0), (30, 0, False, 0)],
    ('130-64', False, True): [(0, 0, True, 0), (0, 0, True, 0), (1, 0, True, 0), (27, 0, True, 0), (30, 0, False, 0), (30, 0, False, 0)],
    ('130-64', True, False): [(30, 0, True, 1), (30, 0, True, 0), (30, 0, True, 0), (30, 0, True, 0), (30, 0, False, 0), (30, 0, False, 0)],
    ('130-64', True, True): [(0, 0, True, 0), (0, 0, True, 0), (1, 0, True, 0), (26, 0, True, 0), (30, 0, False, 0), (30, 0, False, 0)],
    ('192-5x17x64', False, False): [(30, 0, True, 3), (30, 0, True, 3), (30, 0, True, 3), (30, 0, True, 3), (30, 0, False, 0), (30, 0, False, 3)],
    ('192-5x17x64', False, True): [(0, 0, True, 2), (0, 0, True, 2), (1, 0, True, 0), (11, 0, True, 1), (30, 0, False, 2), (30, 0, False, 0)],
    ('192-5x17x64', True, False): [(30, 0, True, 3), (30, 0, True, 3), (30, 0, True, 3), (30, 0, True, 3), (30, 0, False, 0), (30, 0, False, 2)],
    ('192-5x17x64', True, True): [(0, 0, True, 2), (0, 0, True, 2), (1, 0, True, 0), (11, 0, True, 1), (30, 0, False, 2), (30, 0, False, 2)],
    ('1024-64x7', False, False): [(8, 0, True, 2), (8, 0, True, 2), (8, 0, True, 1), (8, 0, False, 1), (8, 0, False, 1), (8, 0, False, 2)],
    ('1024-64x7', False, True): [(0, 0, True, 1), (0, 0, True, 1), (1, 0, True, 1), (8, 0, False, 1), (8, 0, False, 1), (8, 0, False, 1)],
    ('1024-64x7', True, False): [(8, 0, True, 2), (8, 0, True, 2), (8, 0, True, 1), (8, 0, False, 1), (8, 0, False, 1), (8, 0, False, 2)],
    ('1024-64x7', True, True): [(0, 0, True, 1), (0, 0, True, 1), (1, 0, True, 1), (8, 0, False, 1), (8, 0, False, 1), (8, 0, False, 1)],
    ('nosoln-129', False, False): [(2, 1, False, 0), (30, 0, False, 2), (0, 1, False, 0), (30, 0, True, 2)],
    ('nosoln-129', False, True): [(2, 1, False, 0), (24, 0, True, 0), (0, 1, False, 0), (0, 0, True, 1)],
    ('nosoln-129', True, False): [(2, 1, False, 0), (30, 0, False, 2), (0, 1, False, 0), (30, 0, True, 2)],
    ('nosoln-129', True, True): [(2, 1, False, 0), (23, 0, True, 0), (0, 1, False, 0), (0, 0, True, 1)],
    ('nosoln-130', False, False): [(15, 1, False, 0), (25, 1, False, 0), (30, 0, False, 0)],
    ('nosoln-130', False, True): [(10, 1, False, 0), (25, 1, False, 0), (30, 0, False, 0)],
    ('nosoln-130', True, False): [(30, 0, False, 1), (30, 0, False, 0), (30, 0, False, 0)],
    ('nosoln-130', True, True): [(30, 0, False, 0), (30, 0, False, 0), (30, 0, False, 0)],
    ('tol', False, False): [(15, 0, True, 0), (0, 0, False, 1), (30, 0, False, 2)],
    ('tol', False, True): [(0, 0, False, 0), (0, 0, False, 1), (1, 0, False, 0)],
    ('tol', True, False): [(15, 0, True, 0), (0, 0, False, 1), (30, 0, False, 2)],
    ('tol', True, True): [(0, 0, False, 0), (0, 0, False, 1), (1, 0, False, 0)],
}
PIN_KEYS = sorted(PINS)
PIN_IDS = ["%s-%s-%s" % (b, "stable" if s else "ell", "feas" if f else "optim") for b, s, f in PIN_KEYS]


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_lmi_streamed_h.c"
    src.write_text('#include "ellhip_batch_lmi_streamed.h"\n'
                   "int main(void) { ellhip_batch_lmi *o = 0; double g = 0.0;\n"
                   "    return ellhip_batch_lmi_create_streamed(&o, 1, 1, 1, 0, 0, 1, 0, 0, -1) +\n"
                   "           ellhip_batch_lmi_optim_streamed(0, o, &g, 0, 0.0, 0, 0, 0, 0) +\n"
                   "           ellhip_batch_lmi_feas_streamed(0, o, 0, 0.0, 0, 0, 0, 0) +\n"
                   "           ellhip_batch_lmi_optim_streamed_stable(0, o, &g, 0, 0.0, 0, 0, 0, 0) +\n"
                   "           ellhip_batch_lmi_feas_streamed_stable(0, o, 0, 0.0, 0, 0, 0, 0) +\n"
                   "           ELLHIP_BATCH_STREAMED_NMAX + ELLHIP_BATCH_LMI_MMAX; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])
    text = open(HEADER).read()
    for sibling in ("ellhip_batch_lmi.h", "ellhip_batch_streamed.h", "ellhip_batch_streamed_stable.h"):
        assert f'#include "{sibling}"' in text


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    assert declared_functions() == sorted(NAMES) == sorted(capi.BATCH_LMI_STREAMED_EXPORTS)
    others = (capi.EXPORTS + capi.SVM_EXPORTS + capi.BATCH_LMI_EXPORTS + capi.BATCH_LOWPASS_EXPORTS + capi.BATCH_SVM_EXPORTS +
              capi.LMI_LOOP_EXPORTS + capi.BATCH_STABLE_LOOP_EXPORTS + capi.BATCH_STREAMED_EXPORTS +
              capi.BATCH_LOWPASS_STREAMED_EXPORTS + capi.BATCH_STREAMED_STABLE_EXPORTS +
              capi.BATCH_LOWPASS_STREAMED_STABLE_EXPORTS + capi.BATCH_SVM_STREAMED_EXPORTS)
    assert not set(NAMES) & set(others)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_sources_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_lmi_streamed_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_lmi_streamed.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    new = main.index('#include "batch_lmi_streamed_capi.inc.hpp"')
    for dep in ("batch_lmi_capi.inc.hpp", "batch_loop_capi.inc.hpp"):
        assert main.index(f'#include "{dep}"') < new
    inc = open(os.path.join(pkg.build.CSRC, "batch_lmi_streamed_capi.inc.hpp")).read()
    assert "batch_lmi_run(" in inc and "BATCH_ENGINE_STREAMED)" in inc and "BATCH_ENGINE_STREAMED_STABLE)" in inc
    assert "batch_loop_run<BatchLmiOracle>" in open(os.path.join(pkg.build.CSRC, "batch_lmi_capi.inc.hpp")).read()
    driver = open(os.path.join(pkg.build.CSRC, "batch_loop_capi.inc.hpp")).read()
    assert "k_batch_streamed_loop<Oracle>" in driver and "k_batch_streamed_loop_stable<Oracle>" in driver


def test_python_mirror_picks_the_entry_point_by_handle():
    import ellalgo_rs_amd as pkg
    from ellalgo_rs_amd.batch_lmi import _loop_entry

    class Handle:
        def __init__(self, variant, streamed):
            self.variant = variant
            if streamed is not None:
                self.is_streamed = streamed

    ell, stable = pkg.capi.SPACE_ELL, pkg.capi.SPACE_ELL_STABLE
    for name in ("ellhip_batch_lmi_optim", "ellhip_batch_lmi_feas"):
        assert _loop_entry(Handle(ell, None), name) == name
        assert _loop_entry(Handle(stable, None), name) == name + "_stable"
        assert _loop_entry(Handle(ell, True), name) == name + "_streamed"
        assert _loop_entry(Handle(stable, True), name) == name + "_streamed_stable"
    assert callable(pkg.BatchLmiProblem.streamed)


def test_python_mirror_checks_a_shared_pencil_before_the_library():
    import ellalgo_rs_amd as pkg
    f = np.zeros((5, 2, 2))
    with pytest.raises(ValueError):
        pkg.BatchLmiProblem.streamed([np.zeros((3, 5, 2, 2))], c=np.zeros((3, 5)), shared=True)   # a pencil per problem
    with pytest.raises(ValueError):
        pkg.BatchLmiProblem.streamed([f], shared=True)   # nothing tells B
    with pytest.raises(ValueError):
        pkg.BatchLmiProblem.streamed([f], mat_b=[np.zeros((3, 3, 3))], shared=True)


def test_cpp_mirror_offers_the_streamed_form(tmp_path):
    import ellalgo_rs_amd as pkg
    host = os.path.join(pkg.build.HOST_DIR, "ellhip")
    src = tmp_path / "streamed_lmi.cpp"
    src.write_text('#include "batch_lmi_hip.hpp"\n'
                   "using namespace ellhip;\n"
                   "std::size_t f(const std::vector<LmiProblem>& p, EllStableBatchStreamedHip& s, EllBatchStreamedHip& e,\n"
                   "              EllStableBatchHip& l, EllBatchHip& q, Arr& gamma) {\n"
                   "    BatchLmiHip a = BatchLmiHip::streamed(p, 300, {64, 3});\n"
                   "    BatchLmiHip c = BatchLmiHip::streamed_shared(p, 300, {64, 3});\n"
                   "    BatchLmiHip b(p, 100, {4});\n"
                   "    return a.optim(s, gamma, Options(10, 1e-8)).niter[0] + a.optim(e, gamma, Options(10, 1e-8)).niter[0] +\n"
                   "           c.feas(s, Options(10, 1e-8)).niter[0] + c.feas(e, Options(10, 1e-8)).niter[0] +\n"
                   "           b.optim(l, gamma, Options(10, 1e-8)).niter[0] + b.optim(q, gamma, Options(10, 1e-8)).niter[0] +\n"
                   "           b.feas(l, Options(10, 1e-8)).niter[0] + b.feas(q, Options(10, 1e-8)).niter[0];\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", host, str(src)])
    mirror = open(os.path.join(host, "batch_lmi_hip.hpp")).read()
    for name in NAMES:
        assert name in mirror


def test_create_refuses_before_it_looks_for_a_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    INVALID = pkg.capi.E_INVALID

    def create(n, B=2, J=1, m=(2,), f=True, marr=True, shared=0, entry="ellhip_batch_lmi_create_streamed"):
        h = C.c_void_p(12345)
        ms = np.array(m, dtype=np.int64)
        flat = np.zeros(8)   # never read: every call here is answered before the pencils are looked at
        args = [C.byref(h), B, n, J, p(ms) if marr else None, p(flat) if f else None]
        args += ([shared] if entry.endswith("_streamed") else []) + [None, None, -1]
        rc = getattr(lib, entry)(*args)
        assert rc < 0 and h.value is None and lib.ellhip_last_error()
        return rc, lib.ellhip_last_error().decode()

    for n in (0, 1025, -3):
        for shared in (0, 1):
            rc, msg = create(n, shared=shared)
            assert rc == INVALID and "1024" in msg
    assert create(5, B=0)[0] == INVALID
    assert create(5, J=0)[0] == INVALID and create(5, J=9, m=(2,) * 9)[0] == INVALID
    assert create(5, marr=False)[0] == INVALID and create(5, f=False)[0] == INVALID
    assert create(5, m=(0,))[0] == INVALID and create(5, m=(65,))[0] == INVALID
    # the same order as ellhip_batch_lmi_create: the shape before the pointers, the pointers before the block sizes
    assert "1024" in create(1025, J=0, f=False, m=(65,))[1] and "blocks" in create(5, J=0, f=False, m=(65,))[1]
    assert "NULL" in create(5, f=False, m=(65,))[1]
    # the pencils as stored: B of them are too large where one shared pencil is not
    big = dict(B=3000, J=8, m=(64,) * 8)
    assert create(1024, f=True, **big)[0] == pkg.capi.E_NOMEM
    # the LDS engine's constructor keeps its own bound
    rc, msg = create(129, entry="ellhip_batch_lmi_create")
    assert rc == INVALID and "128" in msg
    if lib.ellhip_device_count() > 0:
        return
    for n in (1, 128, 129, 1024):
        assert create(n)[0] == pkg.capi.E_NODEVICE
        assert create(n, shared=1)[0] == pkg.capi.E_NODEVICE
    assert create(1024, shared=1, **big)[0] == pkg.capi.E_NODEVICE
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchLmiProblem.streamed([np.zeros((2, 200, 3, 3))], c=np.zeros((2, 200)))


def test_no_handle_means_a_refusal_not_a_fallback():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    gamma = np.full(2, 0.3)
    x = np.full((2, 129), np.nan)
    has = np.full(2, 7, dtype=np.int32)
    niter = np.full(2, 7, dtype=np.int64)
    status = np.full(2, 7, dtype=np.int32)
    for name in NAMES[1:]:
        head = (None, None) + (() if "feas" in name else (p(gamma),))
        assert getattr(lib, name)(*head, 10, 1e-8, p(x), p(has), p(niter), p(status)) == pkg.capi.E_INVALID
        assert lib.ellhip_last_error()
    assert np.isnan(x).all() and (gamma == 0.3).all() and (has == 7).all() and (niter == 7).all() and (status == 7).all()


def test_lds_needs_follow_the_header():
    """tests/cpp/lmi_streamed_loop_lds_check.hip: both loops' layout functions at every 1 <= n <= 1024 and 1 <= M <= 64, on
    the host"""
    import ellalgo_rs_amd as pkg
    os.makedirs(OUT, exist_ok=True)
    src, exe = os.path.join(CPP, "lmi_streamed_loop_lds_check.hip"), os.path.join(OUT, "lmi_streamed_loop_lds_check")
    deps = [src] + [os.path.join(pkg.build.CSRC, f) for f in pkg.build.HEADERS]
    if _newer(exe, deps):
        subprocess.check_call([pkg.build._hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall",
                               "-Werror", "-Wno-unused-function", "-I", pkg.build.CSRC, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("lmi_streamed_loop_lds_check: ok"), (r.returncode, r.stdout, r.stderr)
    ell, stable, assess = map(int, re.search(r"bytes at n = 1024, M = 64: (\d+) \(Ell\) (\d+) \(EllStable\) (\d+) \(assess\)",
                                             r.stdout).groups())
    assert ell == 8 * (5128 + 6289) == 8 * 11417 and stable == 8 * (4168 + 6289) == 8 * 10457 and assess == 8 * (6289 + 1024)
    assert ell > 64 * 1024 and stable > 64 * 1024   # both need the opt-in
    header = open(HEADER).read()
    assert "89.2 KiB" in header and "81.7 KiB" in header and "57.1 KiB" in header
    assert (round(ell / 1024, 1), round(stable / 1024, 1), round(assess / 1024, 1)) == (89.2, 81.7, 57.1)


# ---- the CPU runs the GPU tests lean on -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PIN_KEYS, ids=PIN_IDS)
def test_reference_pins(key):
    bid, stable, feas = key
    n, ms, who, max_iters, tol, recs = cases.batch_records(bid, stable, feas)
    got = [(r["niter"], r["status"], r["x"] is not None, r["idx"]) for r in recs]
    assert got == PINS[key]
    for r in recs:
        assert len(r["stations"]) == len(r["rows"]) and -1 <= r["idx"] <= len(ms)
        assert r["niter"] <= max_iters and r["mq"].size and r["xc"].shape == (n,)


def all_records():
    for bid, stable, feas in PIN_KEYS:
        n, ms, who, max_iters, tol, recs = cases.batch_records(bid, stable, feas)
        for r in recs:
            yield bid, stable, feas, ms, max_iters, tol, r


def test_the_pinned_set_covers_what_the_gpu_tests_claim():
    kinds, rows, rows_of_64, found_at, ends = set(), set(), set(), set(), set()
    for bid, stable, feas, ms, max_iters, tol, r in all_records():
        J = len(ms)
        for st, row in zip(r["stations"], r["rows"]):
            kinds.add("block" if st < J else "objective" if st == J else "passed")
            if st < J and ms[st] == 64:
                rows_of_64.add(row)
            if st < J:
                assert 0 <= row < ms[st]
                rows.add(row)
        if feas and r["x"] is not None:
            found_at.add(r["niter"])
        if r["status"] == NOSOLN:
            ends.add("nosoln")
        elif feas and r["x"] is not None:
            ends.add("found")
        elif r["niter"] == max_iters:
            ends.add("max_iters")
        else:
            assert r["tsq"] < tol and tol > 0.0 and bid == "tol"
            ends.add("tol")
    assert kinds == {"block", "objective", "passed"}
    assert 0 in rows and 63 in rows_of_64 and any(0 < row < 63 for row in rows_of_64), (sorted(rows), sorted(rows_of_64))
    assert any(k > 0 for k in found_at) and 0 in found_at, sorted(found_at)
    assert ends == {"nosoln", "found", "max_iters", "tol"}
    # on both spaces
    for stable in (False, True):
        mine = [r for _, s, _, _, _, _, r in all_records() if s == stable]
        assert any(r["status"] == NOSOLN for r in mine)


def test_the_tolerance_comes_from_the_middle_of_the_runs_own_trace():
    for stable in (False, True):
        full = cases.record(stable, False, 0, 129, (64, 3), 1.5)
        tol = cases.mid_tol(stable, False)
        cut = cases.batch_records("tol", stable, False)[-1][0]
        k = len(full["tsq_trace"]) // 2
        assert full["niter"] == 30 and 0 < cut["niter"] <= k and cut["status"] == SUCCESS
        assert cut["tsq_trace"] == full["tsq_trace"][:cut["niter"] + 1]   # the same run, ended early
        assert cut["tsq"] < tol and all(v >= tol for v in cut["tsq_trace"][:-1])


def test_equal_blocks_are_family_b():
    import batch_lmi_reference as ref
    fs, bs, c = cases.problem(3, 7, (4, 4))
    rf, rb, rc = ref.family_b(3, 7, 4, 2)
    assert all(np.array_equal(a, b) for a, b in zip(fs, rf)) and all(np.array_equal(a, b) for a, b in zip(bs, rb))
    assert np.array_equal(c, rc)
    d, h = cases.boundary(3, 7, (4, 4))
    assert cases.min_eig(fs, bs, 0.999 * h * d) > 0.0 > cases.min_eig(fs, bs, 1.001 * h * d)
