"""CPU: the restatement of bsearch over BSearchAdaptor (tests/batch_bsearch_reference.py) reproduces the reference's pin
(true, 34) of src/example3.rs:82-84; MyOracle3's four expressions against the family's folds; the conditions the GPU tests
rely on in the seeded family; include/ellhip_batch_bsearch.h is valid C99, libellhip.so exports what it declares, the binding
types it; bad arguments are refused before a device is looked for."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import batch_bsearch_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_bsearch.h")
NAMES = ["ellhip_batch_linfeas_" + s for s in ("create", "destroy", "set_chunk", "set_target", "state", "assess_feas", "feas",
                                               "feas_stable", "bsearch", "bsearch_stable")]
WIDE, SHORT = (2000, 1e-8), (25, 1e-8)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- the pin ------------------------------------------------------------------------------------------------------------------
def test_pin_on_ell():
    r = ref.pin(False)
    assert (r["feasible"], r["niter"]) == (True, 34)                                   # src/example3.rs:83-84
    assert r["upper"] == -7.99974201945588 and r["rounds"] == 352 and sum(r["ends"]) == 34 and r["ends"][3] == 0
    assert r["idx"] in range(4) and abs(r["target"] - r["upper"]) < 4e-8      # the last probe's gamma


def test_pin_on_ellstable():
    r = ref.pin(True)
    assert (r["feasible"], r["niter"]) == (True, 34)
    assert r["upper"] == -7.999930460937321 and r["rounds"] == 405 and sum(r["ends"]) == 34
    assert r["upper"] != ref.pin(False)["upper"]


def test_pin_space_is_untouched_apart_from_xc():
    for stable in (False, True):
        r, fresh = ref.pin(stable), ref.space_of(stable, [0.0, 0.0])
        assert np.array_equal(r["mq"], fresh.mq) and r["kappa"] == fresh.kappa and r["tsq"] == fresh.tsq
        x, y = r["xc"]
        assert max(ref.ex3_expressions(x, y, r["upper"])) <= 0.0          # the last feasible probe's point


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def sweep():
    rng = np.random.default_rng(7)
    special = [0.0, -0.0, 1.0, -1.0, 2.0, 3.0, -2.0, -3.0, 1.5, 0.5, 1e-300, -1e-300, 5e-324, -5e-324, 1e300, -1e300,
               1.7976931348623157e308 / 4, 1.0 / 3.0, -2.0 / 3.0]
    pts = [(x, y) for x in special for y in special]
    pts += [tuple(p) for p in rng.uniform(-10.0, 10.0, (4000, 2))]
    pts += [tuple(p) for p in rng.standard_normal((2000, 2)) * 10.0 ** rng.integers(-12, 12, (2000, 1))]
    pts += [(3.0 * t, 2.0 * t) for t in rng.uniform(-5.0, 5.0, 500)]              # 2 x - 3 y cancels
    return pts


def test_reference_expressions_against_the_folds():
    """bit for bit for every finite x, signed zeros included, with a non-zero target; with a zero target row 3 may differ
    in the sign of a zero fj, which is not > 0.0 and is never handed out (csrc/batch_linfeas_kernels.hpp)"""
    targets = [-1e100, -7.9997, 3.25, 1e-310, 0.0, -0.0]
    omega = ref.LinFeas(ref.EX3_A, ref.EX3_C)
    n_zero_sign = 0
    for x, y in sweep():
        f = omega.folds([x, y])
        assert [bits(float(v)) for v in f] == [bits(ref.fold_scalar(row, (x, y))) for row in ref.EX3_A]
        for target in targets:
            want = ref.ex3_expressions(x, y, target)
            got = [float(f[j]) - (target if j == 3 else ref.EX3_C[j]) for j in range(4)]
            for j in range(4):
                if bits(got[j]) != bits(want[j]):
                    assert j == 3 and target == 0.0 and got[j] == 0.0 and want[j] == 0.0, (x, y, target, j)
                    n_zero_sign += 1
                assert (got[j] > 0.0) == (want[j] > 0.0)
    assert n_zero_sign > 0          # the exception exists: x = -0.0, y = 0.0


def test_oracle_walks_like_the_reference():
    """MyOracle3::assess_feas as written (src/example3.rs:24-55) against the table form, cursor and answers"""
    rng = np.random.default_rng(11)
    omega = ref.LinFeas(ref.EX3_A, ref.EX3_C)
    idx, target = -1, -1e100
    grads = [(-1.0, 0.0), (0.0, -1.0), (1.0, 1.0), (2.0, -3.0)]
    seen = set()
    for step in range(3000):
        if step % 7 == 3:
            target = float(rng.uniform(-12.0, 4.0))
            omega.update(target)
        x, y = (float(v) for v in rng.uniform(-3.0, 3.0, 2) * (0.1 if step % 3 else 1.0))
        want = None
        for _ in range(4):
            idx += 1
            if idx == 4:
                idx = 0
            fj = ref.ex3_expressions(x, y, target)[idx]
            if fj > 0.0:
                want = (grads[idx], fj)
                break
        got = omega.assess_feas([x, y])
        assert omega.idx == idx
        assert (got is None) == (want is None)
        if got is not None:
            assert tuple(got[0]) == want[0] and bits(got[1]) == bits(want[1])
        seen.add(None if want is None else idx)
    assert seen == {None, 0, 1, 2, 3}


# ---- the family the GPU tests lean on -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", [False, True], ids=["ell", "stable"])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_family_takes_all_four_probe_endings(n, stable):
    """at the option sets of tests/test_gpu_batch_bsearch.py, over 40 members: no device comparison passes vacuously"""
    wide, short = ref.runs(n, 40, stable, WIDE), ref.runs(n, 40, stable, SHORT)
    for r in (wide, short):
        assert r["feasible"].all() and set(r["niter"]) == {33}
        assert (r["ends"].sum(axis=1) == 33).all()
    e = wide["ends"].sum(axis=0)
    assert e[ref.END_FEASIBLE] >= 500 and e[ref.END_STATUS] >= 250 and e[ref.END_TOL] >= 100 and e[ref.END_MAX] == 0
    assert short["ends"].sum(axis=0)[ref.END_MAX] >= 50                   # (93 to 482 over these six cases)
    assert wide["round0"] > 0 and short["round0"] > 0                     # a probe that is feasible at round 0 exists
    assert len(set(wide["rounds"])) > 20 and len(set(wide["upper"])) == 40


@pytest.mark.parametrize("stable", [False, True], ids=["ell", "stable"])
def test_family_at_n16(stable):
    r = ref.runs(16, 17, stable, (40, 1e-8))
    e = r["ends"].sum(axis=0)
    assert r["feasible"].all() and set(r["niter"]) == {33}
    assert e[ref.END_FEASIBLE] > 100 and e[ref.END_MAX] > 50 and e[ref.END_STATUS] > 0


def test_large_shapes_have_the_rows_the_limit_allows():
    a, c, xc0 = ref.family(0, 128)
    assert a.shape == (259, 128) and c.shape == (259,) and xc0.shape == (128,)


def test_records_are_read_only():
    r = ref.run(3, 2, False, SHORT)
    with pytest.raises(ValueError):
        r["xc"][0] = 1.0
    with pytest.raises(ValueError):
        ref.family(3, 2)[0][0, 0] = 1.0


# ---- the surface --------------------------------------------------------------------------------------------------------------
def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "batch_bsearch_h.c")])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    assert declared_functions() == sorted(NAMES)
    assert pkg.batch_bsearch.BATCH_BSEARCH_NAMES == sorted(NAMES)
    others = [name for key, names in vars(pkg.capi).items() if key.endswith("EXPORTS") for name in names]
    assert len(others) > 150 and not set(NAMES) & set(others)            # capi's lists mirror the other headers


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.batch_bsearch._load(), name).argtypes is not None


def test_kernels_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    for f in ("batch_linfeas_kernels.hpp", "batch_linfeas_capi.inc.hpp"):
        assert f in pkg.build.HEADERS
    assert "ellhip_batch_bsearch.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_linfeas_capi.inc.hpp")).read()
    assert main.index('#include "batch_loop_capi.inc.hpp"') < main.index('#include "batch_linfeas_capi.inc.hpp"')
    assert '#include "batch_linfeas_kernels.hpp"' in inc and "batch_loop_run<BatchLinFeasOracle" in inc
    assert pkg.BatchLinFeasProblem is not None and "BatchLinFeasProblem" in pkg.__all__


def test_invalid_arguments_and_no_device():
    import ellalgo_rs_amd as pkg
    lib, E = pkg.batch_bsearch._load(), pkg.capi.E_INVALID
    h = C.c_void_p()
    a, c = np.array(ref.EX3_A), np.array(ref.EX3_C)
    p = lambda arr: None if arr is None else arr.ctypes.data_as(C.c_void_p)

    def create(B=2, n=2, J=4, a=a, c=c, shared=1):
        return lib.ellhip_batch_linfeas_create(C.byref(h), B, n, J, p(a), p(c), shared, -1)

    bad = [dict(B=0), dict(B=-1), dict(B=(1 << 24) + 1), dict(n=0), dict(n=129), dict(J=0), dict(J=513), dict(a=None),
           dict(c=None)]
    for args in bad:
        h.value = 0xdead
        assert create(**args) == E and not h.value, args
        assert lib.ellhip_last_error()
    assert lib.ellhip_batch_linfeas_create(None, 2, 2, 4, p(a), p(c), 1, -1) == E
    v, iv = np.full(2, 0.25), np.full(2, 7, dtype=np.int32)
    assert lib.ellhip_batch_linfeas_set_chunk(None, 8) == E
    assert lib.ellhip_batch_linfeas_set_target(None, p(v)) == E
    assert lib.ellhip_batch_linfeas_state(None, p(iv), p(v)) == E
    assert lib.ellhip_batch_linfeas_assess_feas(None, p(v), p(v), p(v), p(iv)) == E
    feas, niter, rounds = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int64), np.full(2, 7, dtype=np.int64)
    up, lo, hi = np.full(2, 7.0), np.full(2, -1.0), np.full(2, 1.0)
    for name in ("ellhip_batch_linfeas_feas", "ellhip_batch_linfeas_feas_stable"):
        assert getattr(lib, name)(None, None, 10, 1e-8, None, p(feas), p(niter), p(iv)) == E
    for name in ("ellhip_batch_linfeas_bsearch", "ellhip_batch_linfeas_bsearch_stable"):
        assert getattr(lib, name)(None, None, p(lo), p(hi), 10, 1e-8, 10, 1e-8, p(feas), p(niter), p(up), p(rounds), None) == E
        assert lib.ellhip_last_error()
    assert (feas == 7).all() and (niter == 7).all() and (up == 7.0).all() and (rounds == 7).all() and (iv == 7).all()
    lib.ellhip_batch_linfeas_destroy(None)
    if lib.ellhip_device_count() > 0:   # (on a GPU machine: the same arguments create a handle)
        for shared, (aa, cc) in ((1, (a, c)), (0, (np.tile(a, (2, 1, 1)), np.tile(c, (2, 1))))):
            assert create(a=aa, c=cc, shared=shared) == 0 and h.value
            assert lib.ellhip_batch_linfeas_set_chunk(h, 0) == E and lib.ellhip_batch_linfeas_set_chunk(h, 4097) == E
            assert lib.ellhip_batch_linfeas_set_chunk(h, 4096) == 0
            lib.ellhip_batch_linfeas_destroy(h)
        return
    h.value = 0xdead
    assert create() == pkg.capi.E_NODEVICE and not h.value
    assert b"no HIP device" in lib.ellhip_last_error()
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchLinFeasProblem(a, c, 2)
    with pytest.raises(ValueError):
        pkg.BatchLinFeasProblem(a, c)                  # a shared table needs B
    with pytest.raises(ValueError):
        pkg.BatchLinFeasProblem(a, c[:3], 2)
    with pytest.raises(ValueError):
        pkg.BatchLinFeasProblem(np.tile(a, (2, 1, 1)), c)
    assert math.isfinite(ref.pin(False)["upper"])
