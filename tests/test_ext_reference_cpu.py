"""CPU: the extended-precision reference and the elementwise comparators of tests/cpp/ext_reference.hpp, which
tests/test_gpu_matrix_core_reference.py holds the FP64 matrix-core passes to.

  * exactness: ref_symm / ref_apply against Python's fractions.Fraction (exact rational arithmetic) on inputs built to cancel;
  * a plain-double evaluation of both operations passes both comparators;
  * six planted defects of the kind a kernel-against-kernel check cannot see are flagged elementwise -- and, planted in a row or
    tile of small scale, are NOT flagged by the suite's norm-wise check (util.rel_inf <= 1e-10): both are asserted, so the test
    documents what was invisible before;
  * pk_vec (the packed operand layout's slot -> vector map) is a permutation and equals the k_pack_operands header's formula.
"""
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cpp_build
from util import TOL, rel_inf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    return cpp_build.build_host_tool("ext_reference_main.cpp")


def _run(tool, tmp_path, mode, dims, arrays, extra=(), out_sizes=None):
    src = tmp_path / "in.bin"
    np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(src)
    args = [tool, mode, *map(str, dims), *map(str, extra), str(src)]
    if out_sizes is None:
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    dst = tmp_path / "out.bin"
    r = subprocess.run(args + [str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    flat = np.fromfile(dst)
    assert flat.size == sum(out_sizes)
    return np.split(flat, np.cumsum(out_sizes)[:-1])


def graded(n, seed, lv=2, np_=24, small=None):
    """Q = D S D, g_v = D^-1 h_v, v_k = D w_k, D = 2^e with e in [-30, 30] (small: (lo, hi), rows whose e is drawn from
    [-30, -20] instead); the strict upper triangle of Q holds NaN: nothing may read it."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-30, 31, n)
    if small:
        e[small[0]:small[1]] = rng.integers(-30, -19, small[1] - small[0])
    d = np.ldexp(1.0, e)
    s = rng.random((n, n)) - 0.5
    q = d[:, None] * s * d[None, :]          # (powers of two: exact)
    q[np.triu_indices(n, 1)] = np.nan
    g = (rng.random((lv, n)) - 0.5) / d
    pend = (rng.random((np_, n)) - 0.5) * d
    cpend = 0.01 * (0.5 + rng.random(np_))
    return e, q, g, pend, cpend


def plain_symm(q, g):
    low = np.tril(np.nan_to_num(q))
    return g @ low.T + g @ np.tril(low, -1)   # rows: sum_c<=r Q[r][c] g[c]; columns: sum_r>c Q[r][c] g[r]


def plain_apply(q, pend, cpend):
    x = np.nan_to_num(q)
    for k in range(len(cpend)):
        x = x - np.outer(cpend[k] * pend[k], pend[k])
    return x


def K_of(n, seg=512):
    return n // 64, (n + seg - 1) // seg


# ---- exactness ----------------------------------------------------------------------------------------------------------
def test_ref_symm_is_exact_to_2_pow_minus_60(tool, tmp_path):
    n, lv = 64, 2
    rng = np.random.default_rng(11)
    q = rng.standard_normal((n, n))
    q[np.triu_indices(n, 1)] = np.nan
    g = rng.standard_normal((lv, n))
    r = n - 1   # the last row has no column terms: y[r] = sum_c Q[r][c] g[c]; make it cancel in the first gradient
    rest = sum(Fraction(q[r, c]) * Fraction(g[0, c]) for c in range(1, n))
    q[r, 0] = float(-rest / Fraction(g[0, 0]))
    hi, lo, S = _run(tool, tmp_path, "symm", (n, n, 0, n, lv), (q, g), out_sizes=[lv * n] * 3)
    worst, cancel = Fraction(0), 0.0
    for v in range(lv):
        for i in range(n):
            y = sum(Fraction(q[i, c]) * Fraction(g[v, c]) for c in range(i + 1))
            y += sum(Fraction(q[rr, i]) * Fraction(g[v, rr]) for rr in range(i + 1, n))
            s = sum(abs(Fraction(q[i, c]) * Fraction(g[v, c])) for c in range(i + 1))
            s += sum(abs(Fraction(q[rr, i]) * Fraction(g[v, rr])) for rr in range(i + 1, n))
            got = Fraction(hi[v * n + i]) + Fraction(lo[v * n + i])
            worst = max(worst, abs(got - y) / s)
            assert abs(Fraction(S[v * n + i]) - s) <= s * Fraction(1, 2 ** 50)
            if y != 0:
                cancel = max(cancel, float(s / abs(y)))
    assert cancel >= 1e12, cancel
    assert worst <= Fraction(1, 2 ** 60), float(worst)


def test_ref_apply_is_exact_to_2_pow_minus_60(tool, tmp_path):
    n, npd = 64, 24
    rng = np.random.default_rng(12)
    q = rng.standard_normal((n, n))
    q[np.triu_indices(n, 1)] = np.nan
    pend = rng.standard_normal((npd, n))
    cpend = 0.01 * (0.5 + rng.random(npd))
    a = -(cpend[:, None] * pend)     # a[k][r], rounded once
    rc, cc = 40, 7                   # x := -sum_k a_k v_k[c], rounded: X is the rounding residue
    q[rc, cc] = float(-sum(Fraction(a[k, rc]) * Fraction(pend[k, cc]) for k in range(npd)))
    hi, lo, M, two, fused = _run(tool, tmp_path, "apply", (n, n, 0, n, npd), (q, pend, cpend), out_sizes=[n * n] * 5)
    worst, cancel = Fraction(0), 0.0
    for r in range(n):
        for c in range(r + 1):
            X = Fraction(q[r, c]) + sum(Fraction(a[k, r]) * Fraction(pend[k, c]) for k in range(npd))
            m = abs(Fraction(q[r, c])) + sum(abs(Fraction(a[k, r]) * Fraction(pend[k, c])) for k in range(npd))
            got = Fraction(hi[r * n + c]) + Fraction(lo[r * n + c])
            worst = max(worst, abs(got - X) / m)
            assert abs(Fraction(M[r * n + c]) - m) <= m * Fraction(1, 2 ** 50)
            if X != 0:
                cancel = max(cancel, float(m / abs(X)))
    assert cancel >= 1e12, cancel
    assert worst <= Fraction(1, 2 ** 60), float(worst)
    # the two plain-double sequences: numpy rounds the product and the difference separately, in recording order
    x = q.copy()
    for k in range(npd):
        x = x - (cpend[k] * pend[k])[:, None] * pend[k][None, :]
    low = np.tril_indices(n)
    assert np.array_equal(two.reshape(n, n)[low], x[low])
    assert np.isnan(two.reshape(n, n)[np.triu_indices(n, 1)]).all()
    # the fused chain rounds once per update: it differs from the two-rounding form somewhere, and by a few ulp at most
    f = fused.reshape(n, n)[low]
    assert (f != x[low]).any() and np.max(np.abs(f - x[low]) / M.reshape(n, n)[low]) <= 2 * npd * 2.0 ** -53


# ---- plain double passes; planted defects -------------------------------------------------------------------------------
N, LV, NPD = 128, 2, 24
SMALL = (32, 48)   # rows / columns forced to small scales: the tile (2, 2) of 16 x 16 blocks is small in both


@pytest.fixture(scope="module")
def case(tool, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("graded")
    e, q, g, pend, cpend = graded(N, 5, LV, NPD, small=SMALL)
    hi, lo, S = _run(tool, tmp, "symm", (N, N, 0, N, LV), (q, g), out_sizes=[LV * N] * 3)
    xh, xl, M, two, fused = _run(tool, tmp, "apply", (N, N, 0, N, NPD), (q, pend, cpend), out_sizes=[N * N] * 5)
    return dict(e=e, q=q, g=g, pend=pend, cpend=cpend, y=hi.reshape(LV, N), X=xh.reshape(N, N), two=two.reshape(N, N),
                fused=fused.reshape(N, N))


def _cmp_symm(tool, tmp_path, c, yhat):
    return _run(tool, tmp_path, "cmp_symm", (N, N, 0, N, LV), (c["q"], c["g"], yhat), extra=K_of(N))


def _cmp_apply(tool, tmp_path, c, qhat):
    return _run(tool, tmp_path, "cmp_apply", (N, N, 0, N, NPD), (c["q"], c["pend"], c["cpend"], qhat))


def test_plain_double_passes_both_comparators(tool, tmp_path, case):
    c = case
    w = _cmp_symm(tool, tmp_path, c, plain_symm(c["q"], c["g"]))
    assert w["ratio"] <= 1.0 and w["index"] == -1, w
    for qhat in (plain_apply(c["q"], c["pend"], c["cpend"]), c["two"], c["fused"]):
        w = _cmp_apply(tool, tmp_path, c, qhat)
        assert w["ratio"] <= 1.0 and w["index"] == -1, w
    # the reference rounded to double is of course inside as well (the baseline of the planted defects below)
    assert _cmp_symm(tool, tmp_path, c, c["y"])["ratio"] <= 1.0 and _cmp_apply(tool, tmp_path, c, np.tril(c["X"]))["ratio"] <= 1.0


def _small_row(e, lo=0):
    return lo + int(np.argmin(e[lo:]))


def test_planted_product_defects_are_flagged_and_were_invisible(tool, tmp_path, case):
    c = case
    q, g, y, e = np.nan_to_num(c["q"]), c["g"], c["y"], c["e"]
    r = _small_row(e, 16)
    assert e[r] <= -20 and e.max() >= 20
    defects = {}
    d = y.copy()                                   # 1. the diagonal counted in both sums
    d[:, r] += q[r, r] * g[:, r]
    defects["diagonal twice"] = (d, r, True)
    d = y.copy()                                   # 2. one 16-column block left out of one row
    d[:, r] -= g[:, 0:16] @ q[r, 0:16]
    defects["block left out"] = (d, r, True)
    d = y.copy()                                   # 3. a strict-upper element read in place of its mirror (8th digit)
    d[:, r] += 1e-8 * q[r, 3] * g[:, 3]
    defects["stale upper element"] = (d, r, True)
    defects["slots exchanged"] = (y[::-1].copy(), 0, False)   # 4. two gradient slots exchanged (every row: visible norm-wise too)
    for name, (yhat, row, invisible) in defects.items():
        w = _cmp_symm(tool, tmp_path, c, yhat)
        assert w["ratio"] > 1.0 and w["index"] % N == row, (name, w)
        if invisible:   # what the suite asserted until now: relative inf-norm per vector
            assert max(rel_inf(yhat[v], y[v]) for v in range(LV)) <= TOL, name


def test_planted_apply_defects_are_flagged_and_were_invisible(tool, tmp_path, case):
    c = case
    q, pend, cpend, X = np.nan_to_num(c["q"]), c["pend"], c["cpend"], np.tril(c["X"])
    assert np.abs(X[SMALL[0]:SMALL[1], SMALL[0]:SMALL[1]]).max() <= 1e-6 * TOL * np.abs(X).max()
    k = 5                                          # 5. one of the NP updates skipped in one 16 x 16 tile
    d = X.copy()
    rows = slice(SMALL[0], SMALL[1])
    d[rows, rows] += np.tril(np.outer(cpend[k] * pend[k, rows], pend[k, rows]))
    w = _cmp_apply(tool, tmp_path, c, d)
    assert w["ratio"] > 1.0 and w["index"] == SMALL[0] * N + SMALL[0], w
    assert rel_inf(d, X) <= TOL
    d = X.copy()                                   # 6. one element with a relative error of 1e-12
    d[40, 35] *= 1.0 + 1e-12
    w = _cmp_apply(tool, tmp_path, c, d)
    assert w["ratio"] > 1.0 and w["index"] == 40 * N + 35, w
    assert rel_inf(d, X) <= TOL
    # a NaN is an error whatever the bound
    d = X.copy()
    d[100, 3] = np.nan
    w = _cmp_apply(tool, tmp_path, c, d)
    assert w["ratio"] == float("inf") and w["index"] == 100 * N + 3, w


# ---- pk_vec ---------------------------------------------------------------------------------------------------------------
def test_pk_vec_is_a_permutation_and_the_headers_slot_formula():
    """'vector 2 p + e sits at slot (p & 3) + 8 ((p & 7) >> 2) + 4 e of tile p >> 3' (k_pack_operands); pk_vec is
    __host__ __device__, so the host's answer is the device's."""
    import ellalgo_rs_amd as pkg
    src, exe = os.path.join(cpp_build.CPP, "pk_vec_check.hip"), os.path.join(cpp_build.OUT, "pk_vec_check")
    os.makedirs(cpp_build.OUT, exist_ok=True)
    if cpp_build._newer(exe, [src] + [os.path.join(pkg.build.CSRC, f) for f in pkg.build.HEADERS]):
        subprocess.check_call([pkg.build._hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
                               "-I", pkg.build.CSRC, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)["pk_vec"]
    assert sorted(got) == list(range(32))
    for v in range(32):
        p, e = v >> 1, v & 1
        t, slot = p >> 3, (p & 3) + 8 * ((p & 7) >> 2) + 4 * e
        assert got[16 * t + slot] == v, (v, t, slot)
