"""The one-step EllStable checker (tests/stable_step_check.py) held to account without a GPU:
(i) its own sums against exact rationals, (ii) the C oracle's step inside every bound at every size and grading the GPU file
uses, (iii) planted defects flagged element by element -- most of them invisible to `rel_inf <= 1e-10` per triangle."""
import math
from fractions import Fraction

import numpy as np
import pytest

import stable_step_check as ssc
from util import TOL, mixed_cut, rel_inf, stable_tau


@pytest.fixture(scope="module")
def calc_of(orc):
    cache = {}
    return lambda n: cache.setdefault(n, orc.Calc(n))


# ------------------------------------------------------------------------------------------------ (i) own sums
@pytest.mark.parametrize("n", [2, 7, 24])
def test_checker_sums_are_exact_on_cancelling_input(n):
    """w~ from rows that cancel 10 to 12 digits, the positive prefix sums and the backward right-hand side: each must be the
    correctly rounded value of the exact rational sum of the double terms."""
    rng = np.random.default_rng(n)
    S = np.tril(rng.standard_normal((n, n)) * np.ldexp(1.0, rng.integers(-20, 21, n))[:, None], -1)
    rows = np.array([math.fsum(S[i, :i].tolist()) for i in range(n)])
    g = rows * (1.0 + 1e-11 * rng.standard_normal(n))           # g_i - sum S[i][:] cancels >= 10 digits
    g[0] = rng.standard_normal()
    wt, mag = ssc.exact_forward(g, S)
    for i in range(n):
        exact = Fraction(g[i]) - sum((Fraction(v) for v in S[i, :i].tolist()), Fraction(0))
        assert wt[i] == float(exact), i
        if i:
            assert abs(wt[i]) <= 1e-10 * mag[i]                  # the cancellation really happened
        assert Fraction(mag[i]) >= (abs(Fraction(g[i])) + sum(abs(Fraction(v)) for v in S[i, :i].tolist())) * (1 - Fraction(n, 2 ** 52))
    gg = rng.random(n) * np.ldexp(1.0, rng.integers(-30, 31, n))
    pre = ssc.exact_prefix(0.37, gg)
    acc = Fraction(0.37)
    for j in range(n):
        acc += Fraction(gg[j])
        assert pre[j] == float(acc)
    d = rng.standard_normal(n)
    cz = rng.standard_normal(n)
    ST = np.ascontiguousarray(S.T)
    for i in range(n - 1):                                       # make the backward rows cancel as well
        cz[i] = -math.fsum((ST[i, i + 1:] * d[i + 1:]).tolist()) * (1.0 + 1e-11)
    rhs, bmag = ssc.exact_backward_rhs(cz, ST, d)
    for i in range(n):
        exact = -Fraction(cz[i]) - sum((Fraction(float(S[j, i] * d[j])) for j in range(i + 1, n)), Fraction(0))
        assert rhs[i] == float(exact), i
        if i < n - 1:
            assert abs(rhs[i]) <= 1e-10 * bmag[i]


# ------------------------------------------------------------------------------ (ii) the oracle inside the bounds
def oracle_case(orc, calc, n, emax, seed, k=8, junk="finite"):
    """The GPU file's sequence on the oracle alone: eight mixed cuts (all entry points, one NoSoln), xc set to 0 before every
    cut but one, every cut checked from the observed states.  Returns the largest observed / bound per stage."""
    buf, e = ssc.graded_factor(n, seed, emax, junk=junk)
    o = orc.OracleEllStable.new_with_matrix(1.5, buf, np.zeros(n))
    rng = np.random.default_rng(seed + 17)
    worst, nsucc = {}, 0
    for i in range(k):
        g = ssc.graded_grad(rng, e)
        kind, b0, b1 = mixed_cut(i, g, stable_tau(o, g), rng)
        if i != ssc.KEEP_XC_AT:
            o.set_xc(np.zeros(n))
        before, xc0, k0 = o.mq.copy(), o.xc.copy(), o.kappa
        st = o.update(kind, g, b0, b1)
        ratios, st_ref = ssc.check_step(calc, before, g, k0, (kind, b0, b1), xc0, o.mq.copy(), o.xc.copy(), o.kappa, o.tsq, st)
        assert not ssc.failures(ratios), (n, emax, i, ratios)
        assert st == st_ref == (1 if i % 8 == 7 else 0)
        nsucc += int(st == 0)
        ssc.merge_max(worst, ratios)
    assert nsucc == k - k // 8
    return worst


@pytest.mark.parametrize("n,emax", ssc.CASES)
def test_oracle_step_is_inside_every_bound(orc, calc_of, n, emax):
    worst = oracle_case(orc, calc_of(n), n, emax, seed=ssc.case_seed(n, emax))
    print(f"oracle n={n} |e|<={emax}: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))   # (shown with -s)
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------- (iii) planted defects
def _normwise_passes(a, b):
    """Would the suite's per-triangle rel_inf <= 1e-10 (plus xc, kappa, tsq) have passed the defective state a against b?"""
    errs = [rel_inf(np.triu(a[0], 1), np.triu(b[0], 1)), rel_inf(np.tril(a[0], -1), np.tril(b[0], -1)),
            rel_inf(np.diag(a[0]), np.diag(b[0])), rel_inf(a[1], b[1]), abs(a[2] - b[2]) / abs(b[2]), abs(a[3] - b[3]) / abs(b[3])]
    return max(errs) <= TOL


def _defect_row(calc_of, defect, n, emax):
    calc = calc_of(n)
    buf, e = ssc.graded_factor(n, 1, emax, junk="finite")
    rng = np.random.default_rng(5)
    small = 3 + int(np.argmin(e[3:n - 3]))
    cut = (0, 0.0, None)
    xc0 = np.zeros(n)
    # two cuts: the second one carries the defect (the scratch triangle of the first is what a stale read would see)
    first = ssc.plain_step(calc, buf, ssc.graded_grad(rng, e), 1.5, cut, xc0)
    g = ssc.graded_grad(rng, e)
    clean = ssc.plain_step(calc, first[0], g, first[2], cut, xc0)
    bad = ssc.plain_step(calc, first[0], g, first[2], cut, xc0, defect=defect, prev_scratch=first[0], small=small)
    r_clean, _ = ssc.check_step(calc, first[0], g, first[2], cut, xc0, *clean)
    assert not ssc.failures(r_clean), (defect, n, emax, r_clean)
    r_bad, _ = ssc.check_step(calc, first[0], g, first[2], cut, xc0, *bad)
    return ssc.failures(r_bad), max(v for v in r_bad.values()), _normwise_passes(bad, clean)


# defect -> (flagged elementwise on the graded input, on the ungraded one; passes rel_inf <= 1e-10 per triangle: graded, ungraded)
DEFECT_TABLE = {
    "stale_w_tile":            ((True, True), (False, True)),
    "fwd_term_dropped":        ((True, True), (False, False)),
    "bwd_term_dropped":        ((True, True), (False, False)),
    "beta2_prev_temp":         ((True, True), (True, False)),
    "D_off_by_one":            ((True, True), (False, False)),
    "scratch_junk":            ((True, True), (True, False)),
    "scratch_of_previous_cut": ((True, True), (False, False)),
}


@pytest.mark.parametrize("defect", ssc.DEFECTS)
def test_planted_defect_is_flagged_elementwise(calc_of, defect):
    """n = 96 with |e| <= 20 and n = 130 ungraded, the defect in the second of two cuts.  Every defect must be flagged on at
    least one of the two inputs (a dropped backward term stands 1e10 above its bound ungraded and 7e3 graded, where most of it
    is absorbed: both kinds of input are needed); the table also pins which of them the norm-wise check of the older tests
    lets through: a stale w (ungraded), beta2 from the previous temp and a surviving junk entry (graded)."""
    rows = [_defect_row(calc_of, defect, 96, 20), _defect_row(calc_of, defect, 130, 0)]
    for (n, em), (fl, worst, nw) in zip(((96, 20), (130, 0)), rows):
        print(f"{defect:24s} n={n} |e|<={em}: flagged {fl or '-'} worst observed/bound {worst:.2e}; "
              f"rel_inf<=1e-10 per triangle would {'PASS' if nw else 'fail'} it")
    flagged = tuple(bool(r[0]) for r in rows)
    assert any(flagged), rows
    assert (flagged, tuple(r[2] for r in rows)) == DEFECT_TABLE[defect], rows


def test_mirrored_restatement_against_the_oracle(orc, calc_of):
    """The multi-cut rule of the GPU file: the plain restatement of the mirrored arithmetic, six cuts unobserved, deviates
    from the oracle by a few roundings per element; four times that is what the GPU may reach."""
    for n in ssc.MULTI_SIZES:
        dev_d, dev_u, _ = ssc.multi_cut_reference(orc, calc_of(n), n)
        print(f"mirrored restatement n={n}: D {dev_d / ssc.U_RND:.2f} u, U {dev_u / ssc.U_RND:.2f} u")
        assert 0.0 < dev_u <= 64 * ssc.U_RND and dev_d <= 64 * ssc.U_RND


def test_mirror_period_sequence_is_well_posed(orc):
    """The 600-cut adaptive sequences of tests/test_gpu_ellstable_mirror_period.py on the oracle: at least half succeed."""
    for n in ssc.PERIOD_SIZES:
        seq = ssc.period_sequence(orc, n, with_nosoln=True)
        assert sum(1 for s in seq.status if s == 0) >= 300 and seq.status[255] == 1
        seq = ssc.period_sequence(orc, n, with_nosoln=False)
        assert all(s == 0 for s in seq.status)
