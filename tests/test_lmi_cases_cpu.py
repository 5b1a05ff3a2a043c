"""CPU: the builders and checkers of tests/lmi_cases.py on the CPU oracle's LDLTMgr / LMIOracle -- they accept a
correct factorisation, and each of five small corruptions of one makes the matching checker fail.  The GPU suite
(tests/test_gpu_lmi_edges.py) relies on exactly these checkers at sizes where no CPU factor is affordable."""
import numpy as np
import pytest

import lmi_cases as lc
from oracle import oracle as O

SIZES = [33, 257, 700, 1057]


def cut_at(a, p, rng):
    """the CPU oracle (LMI0Oracle form) on F(x) = 1.0 * a + 0.0 * f1, f1 = lc.second_matrix(m, rng):
    (f1, storage, wit[:p] zero-extended, ep, g) with pos == (0, p) asserted"""
    m = a.shape[0]
    f1 = lc.second_matrix(m, rng)
    o = O.OracleLMI(np.stack([a, f1]))
    r = o.assess_feas(np.array([1.0, 0.0]))
    assert r is not None and o.ldlt.pos == (0, p)
    v = np.zeros(m)
    v[:p] = o.ldlt.wit[:p]
    return f1, o.ldlt.storage.copy(), v, r[1], r[0]


def run_checkers(a, f1, storage, v, ep, g, p, z):
    return (lc.check_witness(storage, v, p), lc.check_factor_probe(a, storage, p, z), lc.check_ep(a, storage, v, p, ep),
            lc.check_quad(a, v, p, g[0], -1.0), lc.check_quad(f1, v, p, g[1], -1.0))


@pytest.fixture(scope="module")
def cut_1057():
    """the correct output at m = p = 1057, shared (read-only) by the sensitivity tests"""
    rng = np.random.default_rng(1057)
    a = lc.generic_pencil(1057, 1057, rng)
    f1, storage, v, ep, g = cut_at(a, 1057, rng)
    for arr in (a, f1, storage, v, g):
        arr.setflags(write=False)
    return a, f1, storage, v, ep, g


@pytest.mark.parametrize("m", SIZES)
def test_exact_pencil_is_the_cpu_factor_bit_for_bit(m):
    ex = lc.ExactPencil(m, np.random.default_rng(m))
    slab = 256 if m > 256 else (m // 2)
    cases = [(None, 0.0)] + [(k, val) for k in (0, slab - 1, slab, m - 1) for val in (0.0, -2.0 ** -40)]
    for pivot, value in cases:
        case = ex.case(pivot, value)
        ldlt = O.OracleLDLT(m)
        assert ldlt.factorize(case[0]) == (pivot is None)
        lc.check_exact(ldlt.storage, ldlt.pos, None if pivot is None else ldlt.witness(), case)
        if pivot is None:
            np.testing.assert_array_equal(ldlt.sqrt(), lc.expected_sqrt(ldlt.storage))
        else:
            assert case[3] == -value * ex.s[pivot] ** 2 and np.signbit(case[3]) == (value == 0.0)
    a, s, pos, ep = lc.exact_pencil(m, np.random.default_rng(m), pivot=m - 1, value=0.0)
    np.testing.assert_array_equal(a, ex.case(m - 1, 0.0)[0])
    assert pos == (0, m) and np.signbit(ep)


def test_exact_pencil_refuses_a_pivot_it_cannot_represent():
    """at row 7200 the running sum c is above 2^13: c - 2^-40 is no fp64 number and the closed form would not hold"""
    ex = lc.ExactPencil(7201, np.random.default_rng(7201))
    assert ex.c[7199] >= 2.0 ** 13
    with pytest.raises(ValueError):
        ex.case(7200, -2.0 ** -40)
    ex.case(7200, -2.0 ** -38)  # c < 4 * 7201 < 2^15: multiples of 2^-38 are exact at every row


@pytest.mark.parametrize("m,p", [(33, 33), (33, 17), (257, 256), (257, 257), (700, 700), (700, 1), (1057, 1025)])
def test_checkers_accept_the_cpu_oracle(m, p):
    rng = np.random.default_rng(1000 * m + p)
    a = lc.generic_pencil(m, p, rng)
    f1, storage, v, ep, g = cut_at(a, p, rng)
    ratios = run_checkers(a, f1, storage, v, ep, g, p, rng.standard_normal((p, 3)))
    assert max(ratios) <= 0.25, ratios  # the sequential reference sits far inside every bound


def test_checkers_accept_the_cpu_oracle_in_float64_with_the_doubled_bound(cut_1057, monkeypatch):
    """the path the checkers take above LONGDOUBLE_MAX_P, forced at m = 1057"""
    monkeypatch.setattr(lc, "LONGDOUBLE_MAX_P", 0)
    assert lc._acc(1057) == (np.float64, 2.0)
    ratios = run_checkers(*cut_1057, 1057, np.random.default_rng(3).standard_normal((1057, 3)))
    assert max(ratios) <= 0.25, ratios


def test_checkers_accept_the_correct_output_at_1057(cut_1057):
    run_checkers(*cut_1057, 1057, np.random.default_rng(3).standard_normal((1057, 3)))


@pytest.mark.parametrize("float64_path", [False, True])
def test_each_corruption_is_rejected(cut_1057, monkeypatch, float64_path):
    a, f1, storage, v, ep, g = cut_1057
    p = 1057
    if float64_path:
        monkeypatch.setattr(lc, "LONGDOUBLE_MAX_P", 0)
    # a witness entry owned by the second accumulator slot (index >= 1024) lost
    bad = v.copy()
    bad[1030] = 0.0
    with pytest.raises(AssertionError):
        lc.check_witness(storage, bad, p)
    # a witness entry off by 1e-6
    bad = v.copy()
    bad[500] *= 1.0 + 1e-6
    with pytest.raises(AssertionError):
        lc.check_witness(storage, bad, p)
    # a strict-lower storage entry (an L value) off by 1e-6: the largest one of row 900
    bad = storage.copy()
    bad[900, np.argmax(np.abs(storage[900, :900]))] *= 1.0 + 1e-6
    with pytest.raises(AssertionError):
        lc.check_factor_probe(a, bad, p, np.random.default_rng(3).standard_normal((p, 3)))
    # g with one of the eight row chunks of k_lmi_quad left out
    rows_per = (p + 7) // 8
    for chunk in range(8):
        r0, r1 = chunk * rows_per, min(p, (chunk + 1) * rows_per)
        bad_g = g[1] + float(v[r0:r1] @ (f1[r0:r1] @ v))  # g[1] = -v' f1 v
        with pytest.raises(AssertionError):
            lc.check_quad(f1, v, p, bad_g, -1.0)
    # ep that is not the stored pivot
    with pytest.raises(AssertionError):
        lc.check_ep(a, storage, v, p, np.nextafter(ep, np.inf))


def test_one_ulp_in_an_exact_factor_is_rejected():
    m = 1057
    case = lc.exact_pencil(m, np.random.default_rng(m))
    ldlt = O.OracleLDLT(m)
    assert ldlt.factorize(case[0])
    lc.check_exact(ldlt.storage, ldlt.pos, None, case)
    for i, j in ((1040, 3), (3, 1040), (1056, 1056)):  # an L value, a kept T value, a pivot
        bad = ldlt.storage.copy()
        bad[i, j] = np.nextafter(bad[i, j], np.inf)
        with pytest.raises(AssertionError):
            lc.check_exact(bad, ldlt.pos, None, case)
    zero = lc.exact_pencil(m, np.random.default_rng(m), pivot=1024, value=0.0)
    assert not ldlt.factorize(zero[0])
    lc.check_exact(ldlt.storage, ldlt.pos, ldlt.witness(), zero)
    with pytest.raises(AssertionError):
        lc.check_exact(ldlt.storage, ldlt.pos, 0.0, zero)  # +0.0 where the reference returns -0.0
    r = lc.expected_sqrt(case[1])
    assert np.all(np.tril(r, -1) == 0.0) and r[3, 1040] == case[1][1040, 3] * np.sqrt(case[1][3, 3])
