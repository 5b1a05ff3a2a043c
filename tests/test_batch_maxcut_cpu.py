"""CPU: include/ellhip_batch_maxcut.h is valid C99, the binding lists exactly what it declares and libellhip.so exports it,
the kernels are part of the build recipe, the entry points refuse bad arguments before they look for a device and refuse to
run without one (no CPU fallback), the LDS needs of the four loops follow the header's formulas
(tests/cpp/maxcut_loop_lds_check.hip), the restated oracle gives the reference's known answers, and the CPU reference runs
the GPU tests compare against (tests/batch_maxcut_reference.py) are pinned."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_maxcut_reference as ref
from cpp_build import CPP, OUT, _newer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ellhip_batch_maxcut.h")
LOOPS = ["ellhip_batch_maxcut_optim" + s for s in ("", "_stable", "_streamed", "_streamed_stable")]
NAMES = ["ellhip_batch_maxcut_" + s for s in ("create", "destroy", "set_chunk", "assess_optim")] + LOOPS
INF = np.inf


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ellhip_batch_maxcut_[a-z0-9_]+)\s*\(", src)))


def test_header_is_valid_c99(tmp_path):
    src = tmp_path / "batch_maxcut_h.c"
    src.write_text('#include "ellhip_batch_maxcut.h"\nint main(void) { ellhip_batch_maxcut *o = 0; '
                   'ellhip_batch_maxcut_destroy(o); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_lists_what_the_header_declares():
    import ellalgo_rs_amd as pkg
    capi = pkg.capi
    assert declared_functions() == sorted(NAMES)
    assert declared_functions() == sorted(capi.BATCH_MAXCUT_EXPORTS)
    others = [name for key, names in vars(capi).items() if key.endswith("EXPORTS") and key != "BATCH_MAXCUT_EXPORTS"
              for name in names]
    assert len(others) > 150 and set(capi.EXPORTS) <= set(others)
    assert not set(capi.BATCH_MAXCUT_EXPORTS) & set(others)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    import ellalgo_rs_amd as pkg
    lib = C.CDLL(pkg.capi.lib_path())
    assert getattr(lib, name) is not None
    assert getattr(pkg.capi.load(), name).argtypes is not None


def test_kernels_are_in_the_build_recipe():
    import ellalgo_rs_amd as pkg
    assert "batch_maxcut_kernels.hpp" in pkg.build.HEADERS
    assert "batch_maxcut_capi.inc.hpp" in pkg.build.HEADERS
    assert "ellhip_batch_maxcut.h" in pkg.build.PUBLIC_HEADERS
    main = open(os.path.join(pkg.build.CSRC, "ellhip_capi.hip")).read()
    inc = open(os.path.join(pkg.build.CSRC, "batch_maxcut_capi.inc.hpp")).read()
    assert main.index('#include "batch_loop_capi.inc.hpp"') < main.index('#include "batch_maxcut_capi.inc.hpp"')
    assert '#include "batch_maxcut_kernels.hpp"' in inc
    assert inc.count("batch_loop_run<BatchMaxcutOracle>") == 1 and "batch_loop_drive" not in inc   # no second driver
    assert pkg.BatchMaxcutProblem is not None


def test_invalid_arguments_and_no_device():
    import ellalgo_rs_amd as pkg
    lib = pkg.capi.load()
    h = C.c_void_p()
    w = np.zeros((2, 4, 4))

    def create(B, n, tab=w, shared=0):
        return lib.ellhip_batch_maxcut_create(C.byref(h), B, n, None if tab is None else tab.ctypes.data, shared, -1)

    for args in ((0, 4), (-1, 4), ((1 << 24) + 1, 4), (2, 0), (2, -3), (2, 1025), (2, 4, None), (2, 4, None, 1)):
        h.value = 0xdead
        assert create(*args) == pkg.capi.E_INVALID and not h.value, args
        assert lib.ellhip_last_error()
    assert lib.ellhip_batch_maxcut_create(None, 2, 4, w.ctypes.data, 0, -1) == pkg.capi.E_INVALID
    # NULL handles and pointers
    x, gamma, grad = np.zeros((2, 4)), np.zeros(2), np.zeros((2, 4))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ellhip_batch_maxcut_set_chunk(None, 8) == pkg.capi.E_INVALID
    assert lib.ellhip_batch_maxcut_assess_optim(None, p(x), p(gamma), p(grad), None, None, None) == pkg.capi.E_INVALID
    has, niter, status = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int64), np.full(2, 7, dtype=np.int32)
    xb = np.full((2, 4), np.nan)
    gamma[:] = 0.3
    for name in LOOPS:
        assert getattr(lib, name)(None, None, p(gamma), 10, 1e-8, p(xb), p(has), p(niter), p(status)) == pkg.capi.E_INVALID
        assert lib.ellhip_last_error()
    assert np.isnan(xb).all() and (gamma == 0.3).all() and (has == 7).all() and (niter == 7).all() and (status == 7).all()
    lib.ellhip_batch_maxcut_destroy(None)
    if lib.ellhip_device_count() > 0:  # (on a GPU machine: the same arguments create a handle)
        for n, shared in ((4, 0), (4, 1)):
            assert create(2, n, shared=shared) == 0 and h.value
            assert lib.ellhip_batch_maxcut_set_chunk(h, 0) == pkg.capi.E_INVALID
            assert lib.ellhip_batch_maxcut_set_chunk(h, 4097) == pkg.capi.E_INVALID
            assert lib.ellhip_batch_maxcut_set_chunk(h, 4096) == 0
            lib.ellhip_batch_maxcut_destroy(h)
        return
    for n, shared in ((4, 0), (4, 1)):
        h.value = 0xdead
        assert create(2, n, shared=shared) == pkg.capi.E_NODEVICE and not h.value
        assert b"no HIP device" in lib.ellhip_last_error()
    with pytest.raises(pkg.capi.EllHipError):
        pkg.BatchMaxcutProblem(w)
    with pytest.raises(ValueError):
        pkg.BatchMaxcutProblem(w[0])             # a shared table needs B
    with pytest.raises(ValueError):
        pkg.BatchMaxcutProblem(w[:, :3])         # not square
    with pytest.raises(ValueError):
        pkg.BatchMaxcutProblem(w, 3)             # B differs


def test_lds_needs_follow_the_header():
    """tests/cpp/maxcut_loop_lds_check.hip: the four loops' layout functions at every n their engines take, on the host"""
    import ellalgo_rs_amd as pkg
    os.makedirs(OUT, exist_ok=True)
    src, exe = os.path.join(CPP, "maxcut_loop_lds_check.hip"), os.path.join(OUT, "maxcut_loop_lds_check")
    deps = [src] + [os.path.join(pkg.build.CSRC, f) for f in pkg.build.HEADERS]
    if _newer(exe, deps):
        subprocess.check_call([pkg.build._hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall",
                               "-Werror", "-Wno-unused-function", "-I", pkg.build.CSRC, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("maxcut_loop_lds_check: ok"), (r.returncode, r.stdout, r.stderr)
    lds = {int(n): (int(a), int(b)) for n, a, b in re.findall(r"bytes at n = (\d+): (\d+) \(Ell\) (\d+) \(EllStable\)", r.stdout)}
    o128, o1024 = (3 * 128 + 8) | 1, (3 * 1024 + 8) | 1
    assert lds[128] == (8 * (((128 * 129 + 2 * 128 + 8) | 1) + o128), 8 * (((128 * 129 + 3 * 128 + 8) | 1) + o128))
    assert lds[1024] == (8 * (5 * 1024 + 8 + o1024), 8 * (4 * 1024 + 72 + o1024))
    assert max(lds[128] + lds[1024]) <= 159 * 1024
    header = open(HEADER).read()
    for nbytes in lds[128] + lds[1024]:
        assert f"{nbytes / 1024:.1f} KiB" in header, nbytes


# ---- the reference's known answers (src/oracles/maxcut_oracle.rs:57-83) ------------------------------------------------------
def test_reference_known_answers():
    w = np.array([[0.0, 1.0], [1.0, 0.0]])
    x = np.array([1.0, 1.0])
    (g, beta), improved, gamma, cut = ref.assess_optim(w, x, -INF)
    assert improved and gamma == 0.0 and not np.signbit(gamma) and cut == 0.0 and not np.signbit(cut)
    assert beta == 0.0 and np.signbit(beta)
    assert (g == 0.0).all() and np.signbit(g).all()
    (g2, beta2), improved2, gamma2, _ = ref.assess_optim(w, x, gamma)
    assert not improved2 and beta2 == 0.0 and not np.signbit(beta2) and gamma2 == 0.0
    assert (g2 == 0.0).all() and np.signbit(g2).all()


def test_signs_folds_and_the_diagonal():
    assert ref.signs([0.0, -0.0, np.nan, -1e-300, INF, -INF]).tolist() == [1.0, 1.0, -1.0, -1.0, 1.0, -1.0]
    # full rows for the gradient, the upper triangle for the value, no diagonal
    w = np.array([[100.0, 1.0, 2.0], [4.0, 200.0, 8.0], [16.0, 32.0, 300.0]])
    (g, beta), improved, gamma, cut = ref.assess_optim(w, [1.0, -1.0, 1.0], 8.5)
    assert cut == 1.0 + 8.0 and improved and gamma == 9.0 and beta == -9.0
    assert g.tolist() == [-2.0, -24.0, -64.0]
    (g, beta), improved, gamma, cut = ref.assess_optim(w, [1.0, -1.0, 1.0], 9.0)   # a tie is not an improvement
    assert not improved and beta == 9.0 and gamma == 9.0
    # the order of the fold shows: 1e16 + 1 + 1 is 1e16 one add after the other, 1e16 + 2 in any other order
    w = np.zeros((4, 4))
    w[0, 1], w[0, 2], w[0, 3] = 1e16, 1.0, 1.0
    cut = ref.assess_optim(w, [1.0, -1.0, -1.0, -1.0], INF)[3]
    assert cut == 1e16
    w[0, 1], w[0, 3] = 1.0, 1e16
    assert ref.assess_optim(w, [1.0, -1.0, -1.0, -1.0], INF)[3] == 1e16 + 2.0
    # a NaN weight: the value is NaN and never improves
    w[0, 2] = np.nan
    (g, beta), improved, gamma, cut = ref.assess_optim(w, [1.0, -1.0, -1.0, -1.0], -INF)
    assert np.isnan(cut) and not improved and beta == -INF and gamma == -INF and np.isnan(g[0]) and not np.isnan(g[1:]).any()


# ---- the CPU runs the GPU tests lean on ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind,max_iters,ell,stable", ref.ROWS, ids=ref.ROW_IDS)
def test_family_pins(n, kind, max_iters, ell, stable):
    for is_stable, niters in ((False, ell), (True, stable)):
        runs = [ref.solve(s, n, kind, max_iters, ref.TOL, is_stable) for s in range(6)]
        assert tuple(r["niter"] for r in runs) == niters
        for r in runs:
            assert r["niter"] < max_iters and r["status"] == ref.NOSOLN and r["x_best"] is not None   # the first call improves on -inf
            assert r["central"] >= 1 and r["central"] + r["deep"] == r["niter"]   # the last cut is the deep one that fails
        if kind == "mixed":   # long runs: at least half the members, each with central and successful deep cuts
            long_runs = [r for r in runs if r["niter"] >= 20]
            assert 2 * len(long_runs) >= len(runs)
            assert all(r["central"] >= 2 and r["deep"] >= 1 for r in long_runs)
        else:
            assert max(r["niter"] for r in runs) <= 12


def test_max_iters_zero_keeps_everything():
    w, xc0 = ref.weights(1, 16, "mixed")
    space = ref.fresh(xc0)
    r = ref.run(w, 0, ref.TOL, space, gamma=-3.0)
    assert r["x_best"] is None and r["niter"] == 0 and r["gamma"] == -3.0 and r["status"] == ref.SUCCESS
    assert r["kappa"] == ref.KAPPA and np.array_equal(r["xc"], xc0)


def test_records_are_read_only():
    r = ref.solve(3, 16, "mixed", 2000)
    with pytest.raises(ValueError):
        r["xc"][0] = 1.0
    with pytest.raises(ValueError):
        r["x_best"][0] = 1.0
