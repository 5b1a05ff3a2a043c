"""CPU: include/ellhip_batch_bsearch_streamed.h is valid C99, libellhip.so exports what it declares and the binding types it in
a table of its own, the old header's list is unchanged, the new files are in the build recipe, _create_streamed refuses bad
arguments before a device is looked for; and the conditions the GPU cases (tests/batch_bsearch_streamed_cases.py) are there
to cover hold on the reference records, so that no device comparison passes vacuously."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_bsearch_reference as ref
import batch_bsearch_streamed_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_bsearch_streamed.h")
OLD_HEADER = os.path.join(ROOT, "include", "ellhip_batch_bsearch.h")
NAMES = ["ellhip_batch_linfeas_" + s for s in ("create_streamed", "feas_streamed", "feas_streamed_stable", "bsearch_streamed",
                                               "bsearch_streamed_stable")]
OLD_NAMES = ["ellhip_batch_linfeas_" + s for s in ("create", "destroy", "set_chunk", "set_target", "state", "assess_feas",
                                                   "feas", "feas_stable", "bsearch", "bsearch_stable")]


def declared_functions(header):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


# ---- the surface --------------------------------------------------------------------------------------------------------------
def test_header_is_valid_c99():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "batch_bsearch_streamed_h.c")])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    assert declared_functions(HEADER) == sorted(NAMES)
    assert pkg.batch_bsearch.BATCH_BSEARCH_STREAMED_NAMES == sorted(NAMES)
    assert sorted(pkg.batch_bsearch.STREAMED_PROTOTYPES) == sorted(NAMES)
    others = [name for key, names in vars(pkg.capi).items() if key.endswith("EXPORTS") for name in names]
    assert not set(NAMES) & set(others)


def test_old_header_and_its_list_are_unchanged():
    import ellalgo_rs_amd as pkg
    assert declared_functions(OLD_HEADER) == sorted(OLD_NAMES)
    assert pkg.batch_bsearch.BATCH_BSEARCH_NAMES == sorted(OLD_NAMES) == sorted(pkg.batch_bsearch.PROTOTYPES)
    assert not set(NAMES) & set(OLD_NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.batch_bsearch._load(), name).argtypes is not None


def test_prototypes_are_the_counterparts():
    import ellalgo_rs_amd as pkg
    P, S = pkg.batch_bsearch.PROTOTYPES, pkg.batch_bsearch.STREAMED_PROTOTYPES
    assert S["ellhip_batch_linfeas_create_streamed"] == P["ellhip_batch_linfeas_create"]
    for name in ("feas", "bsearch"):
        for suffix in ("_streamed", "_streamed_stable"):
            assert S[f"ellhip_batch_linfeas_{name}{suffix}"] == P[f"ellhip_batch_linfeas_{name}"]


def test_kernels_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    for f in ("batch_linfeas_streamed_kernels.hpp", "batch_linfeas_streamed_capi.inc.hpp"):
        assert f in pkg.build.HEADERS
    assert "ellhip_batch_bsearch_streamed.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_linfeas_streamed_capi.inc.hpp")).read()
    kernels = open(os.path.join(pkg.build.CSRC, "batch_linfeas_streamed_kernels.hpp")).read()
    assert main.index('#include "batch_linfeas_capi.inc.hpp"') < main.index('#include "batch_linfeas_streamed_capi.inc.hpp"')
    assert '#include "batch_linfeas_streamed_kernels.hpp"' in inc
    assert "batch_loop_run<BatchLinFeasOracle, BATCH_DRIVER_OPTIM, /*STREAMED=*/true>" in inc
    assert "batch_bsearch_drive(" in inc                       # the host loop is shared, not copied
    assert "hipMemcpy" not in inc
    for k in ("k_batch_streamed_bsearch", "k_batch_streamed_bsearch_stable", "k_batch_linfeas_assess_wg"):
        assert re.search(r"__launch_bounds__\(1024\) void " + k + r"\(", kernels), k
    assert callable(pkg.BatchLinFeasProblem.streamed)


def test_invalid_arguments_and_no_device():
    import ellalgo_rs_amd as pkg
    lib, E = pkg.batch_bsearch._load(), pkg.capi.E_INVALID
    h = C.c_void_p()
    a, c = np.array(ref.EX3_A), np.array(ref.EX3_C)
    p = lambda arr: None if arr is None else arr.ctypes.data_as(C.c_void_p)

    def create(B=2, n=2, J=4, a=a, c=c, shared=1):
        return lib.ellhip_batch_linfeas_create_streamed(C.byref(h), B, n, J, p(a), p(c), shared, -1)

    bad = [dict(B=0), dict(B=-1), dict(B=(1 << 24) + 1), dict(n=0), dict(n=1025), dict(J=0), dict(J=4097), dict(a=None),
           dict(c=None)]
    for args in bad:
        h.value = 0xdead
        assert create(**args) == E and not h.value, args
        assert lib.ellhip_last_error()
    assert lib.ellhip_batch_linfeas_create_streamed(None, 2, 2, 4, p(a), p(c), 1, -1) == E
    iv = np.full(2, 7, dtype=np.int32)
    feas, niter, rounds = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int64), np.full(2, 7, dtype=np.int64)
    up, lo, hi = np.full(2, 7.0), np.full(2, -1.0), np.full(2, 1.0)
    for name in ("ellhip_batch_linfeas_feas_streamed", "ellhip_batch_linfeas_feas_streamed_stable"):
        assert getattr(lib, name)(None, None, 10, 1e-8, None, p(feas), p(niter), p(iv)) == E
    for name in ("ellhip_batch_linfeas_bsearch_streamed", "ellhip_batch_linfeas_bsearch_streamed_stable"):
        assert getattr(lib, name)(None, None, p(lo), p(hi), 10, 1e-8, 10, 1e-8, p(feas), p(niter), p(up), p(rounds), None) == E
        assert lib.ellhip_last_error()
    assert (feas == 7).all() and (niter == 7).all() and (up == 7.0).all() and (rounds == 7).all() and (iv == 7).all()
    if lib.ellhip_device_count() > 0:   # (on a GPU machine: the limits' own values create a handle)
        big_a, big_c = np.zeros((4096, 1024)), np.zeros(4096)
        assert create(B=1, n=1024, J=4096, a=big_a, c=big_c) == 0 and h.value
        lib.ellhip_batch_linfeas_destroy(h)
        return
    h.value = 0xdead                     # it accepts nothing without a device
    assert create() == pkg.capi.E_NODEVICE and not h.value
    assert b"no HIP device" in lib.ellhip_last_error()
    h.value = 0xdead
    assert create(B=1, n=1024, J=4096, a=np.zeros((4096, 1024)), c=np.zeros(4096)) == pkg.capi.E_NODEVICE and not h.value
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchLinFeasProblem.streamed(a, c, 2)
    with pytest.raises(ValueError):
        pkg.BatchLinFeasProblem.streamed(a, c)         # a shared table needs B


# ---- what the GPU cases cover -------------------------------------------------------------------------------------------------
def test_stock_interval_is_feasible_at_once_past_one_wave():
    """why the cases past n = 64 take other intervals: with (-50, 50) no probe ends any other way than feasible"""
    for n, B in ((65, 3), (129, 2)):
        for stable in (False, True):
            r = ref.runs(n, B, stable, (30, 1e-8), (6, 1e-8))
            assert (r["ends"][:, 1:] == 0).all() and (r["ends"][:, 0] == 6).all()


@pytest.mark.parametrize("stable", [False, True], ids=["ell", "stable"])
@pytest.mark.parametrize("case", [c for c in cases.FAMILY if c.straddles], ids=lambda c: c.id)
def test_straddling_cases_cover_what_they_are_there_for(case, stable):
    w = case.want(stable)
    e = w["ends"].sum(axis=0)
    assert w["feasible"].all() and (w["ends"].sum(axis=1) == w["niter"]).all() and set(w["niter"]) == {case.outer[0]}
    assert e[ref.END_FEASIBLE] > 0 and e[ref.END_STATUS] > 0 and e[ref.END_TOL] == 0     # feasible, and by a failed cut
    if not case.max_end:        # n = 1024: short probes, to keep the CPU record at half a second a member
        assert e[ref.END_MAX] == 0 and (w["rounds"] >= 9).all() and (w["rounds"] <= 11).all()
        return
    assert e[ref.END_MAX] > 0                                                           # ... and by inner_max_iters
    assert (w["rounds"] >= 5 * w["niter"]).any()                                         # long probes
    probes = [q for b in range(case.B) for q in cases.probes_of(case, b, stable)]
    assert sum(calls for calls, _ in probes) == w["rounds"].sum()
    assert any(feasible and calls >= 3 for calls, feasible in probes)                   # a feasible probe after >= 2 cuts
    if case is cases.N129:
        assert any(feasible and calls == 1 for calls, feasible in probes)               # and one that moves no matrix bytes


@pytest.mark.parametrize("case", [c for c in cases.FAMILY if c.straddles and c.max_end], ids=lambda c: c.id)
def test_the_two_spaces_take_different_paths(case):
    assert (case.want(False)["rounds"] != case.want(True)["rounds"]).any()


def test_small_cases_take_all_four_endings():
    """n = 2 and n = 5 with the stock interval, over the members the GPU cases use"""
    for stable in (False, True):
        e = sum(c.want(stable)["ends"].sum(axis=0) for c in cases.FAMILY if c.n <= 5)
        assert (e > 0).all()


@pytest.mark.parametrize("stable", [False, True], ids=["ell", "stable"])
def test_tolerance_case_ends_by_the_tolerance(stable):
    w = cases.TOL_END.want(stable)
    assert (w["ends"][:, ref.END_TOL] > 0).all() and (w["ends"][:, ref.END_FEASIBLE] > 0).all()


def test_second_call_and_no_defer_trick_records_differ():
    c = cases.N129
    for stable in (False, True):
        first, again = c.want(stable, B=3), c.want(stable, B=3, again=0.5)
        assert (again["niter"] > 0).all() and (again["rounds"] > 0).all() and (again["upper"] != first["upper"]).any()
    plain, ndt = c.want(False, B=3), c.want(False, B=3, no_defer_trick=True)
    assert not np.array_equal(plain["xc"].view(np.int64), ndt["xc"].view(np.int64))
