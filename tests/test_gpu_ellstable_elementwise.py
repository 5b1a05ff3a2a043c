"""Every single-handle EllStable kernel form held to the one-step residual bounds of tests/stable_step_check.py.

The older EllStable tests are norm-wise on factors drawn at one scale, or compare one kernel form with another.  Here every
update is checked from what the C ABI shows -- buffer, xc, kappa, tsq before and after -- element by element and on each
element's own scale, on factors graded row by row over 2^-10 .. 2^10 (one case 2^-20 .. 2^20) and on ungraded ones, with NaN
in the scratch triangle for the eager forms (the first forward solve must overwrite all of it; a survivor poisons the scratch
check) and finite junk for the mirrored layout (entering it copies U over the junk).  tests/test_stable_step_check_cpu.py holds
the checker itself to exact rationals, to the oracle and to planted defects.
"""
import numpy as np
import pytest

import stable_step_check as ssc
from util import beta_of, mixed_cut, set_default, stable_tau

pytestmark = pytest.mark.gpu

# (STABLE_SOLVE, STABLE_FACTOR): one launch per block + LDS-transposed factor tiles; persistent solves + row-wise factor update;
# helped solves with the factor tiles pulled inside the backward launch; helped solves + the plain factor kernel; the mirrored layout
FORMS = [(0, 0), (1, 1), (2, 2), (2, 0), (3, 2)]


def _run_form(gpu, orc, calc, n, emax, solve, factor):
    """Eight cuts from util.mixed_cut (tau from the oracle, as in run_mixed_stable): all six EllCalc entry points, the
    parallel cut that falls back to a deep cut with beta < 0, one NoSoln.  Observed after every cut; xc = 0 before every cut
    but one.  Returns the largest observed / bound per stage."""
    capi = gpu.capi
    set_default("STABLE_SOLVE", solve)
    set_default("STABLE_FACTOR", factor)
    seed = ssc.case_seed(n, emax)
    buf, e = ssc.graded_factor(n, seed, emax, junk="finite" if solve == 3 else "nan")
    h = gpu.EllStable.new_with_matrix(1.5, buf, np.zeros(n))
    assert h.get_option(capi.OPT_STABLE_SOLVE) == solve and h.get_option(capi.OPT_STABLE_FACTOR) == factor
    o = orc.OracleEllStable.new_with_matrix(1.5, buf, np.zeros(n))
    rng = np.random.default_rng(seed + 17)
    worst, before = {}, buf
    for i in range(8):
        g = ssc.graded_grad(rng, e)
        kind, b0, b1 = mixed_cut(i, g, stable_tau(o, g), rng)
        if i != ssc.KEEP_XC_AT:
            h.set_xc(np.zeros(n))
            o.set_xc(np.zeros(n))
        xc0, k0 = h.xc(), h.kappa
        assert np.any(xc0 != 0.0) == (i == ssc.KEEP_XC_AT)
        so = o.update(kind, g, b0, b1)
        sg = int(h._update(kind, (g, beta_of(b0, b1))))
        if solve == 3:
            assert h.get_option(capi.OPT_STABLE_MIRRORED) == 1      # (the observer below leaves the layout, the next cut enters it)
        after, xc1 = h.mq, h.xc()
        ratios, st_ref = ssc.check_step(calc, before, g, k0, (kind, b0, b1), xc0, after, xc1, h.kappa, h.tsq(), sg)
        print(f"  n={n} |e|<={emax} form=({solve},{factor}) cut {i}: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items())))
        assert sg == so == st_ref == (1 if i == 7 else 0), (i, sg, so, st_ref)
        assert not ssc.failures(ratios), (n, emax, (solve, factor), i, ratios)
        ssc.merge_max(worst, ratios)
        before = after
    return worst


@pytest.mark.parametrize("n,emax", ssc.CASES)
def test_every_form_is_inside_the_one_step_bounds(gpu, orc, n, emax):
    calc = orc.Calc(n)
    for solve, factor in FORMS:
        worst = _run_form(gpu, orc, calc, n, emax, solve, factor)
        print(f"WORST n={n} |e|<={emax} form=({solve},{factor}): " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))
        assert all(v <= 1.0 for v in worst.values()), ((solve, factor), worst)


@pytest.mark.parametrize("n", ssc.MULTI_SIZES)
def test_six_cuts_inside_the_mirrored_layout(gpu, orc, n):
    """The one-step checks cannot see inside a stretch nobody observes, so this one is a rule, not a derived bound: six cuts
    inside the mirrored layout on the graded factor, then D and U against the oracle, every element relative to itself
    (U' = U prod(1 + beta2 w) does not cancel: no element is excluded).  The allowance is four times what a plain numpy
    restatement of the mirrored arithmetic (ssc.mirrored_run: reference summation order) deviates from the oracle on the same
    cuts -- 8.2 u at n = 129 and 9.6 u at n = 300, u = 2^-53; the margin is for the kernels' other summation order."""
    set_default("STABLE_SOLVE", 3)
    dev_d, dev_u, (buf, kappa, cuts, d_o, u_o) = ssc.multi_cut_reference(orc, orc.Calc(n), n)
    allow = 4.0 * max(dev_d, dev_u)
    h = gpu.EllStable.new_with_matrix(kappa, buf, np.zeros(n))
    assert h.get_option(gpu.capi.OPT_STABLE_SOLVE) == 3
    for kind, g, b0, b1 in cuts:
        assert int(h._update(kind, (g, beta_of(b0, b1)))) == 0
    assert h.get_option(gpu.capi.OPT_STABLE_MIRRORED) == 1
    m = h.mq
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    got_d, got_u = ssc.rel_elementwise(np.diag(m), d_o), ssc.rel_elementwise(np.triu(m, 1), u_o, up)
    print(f"MULTI n={n}: restatement D {dev_d / ssc.U_RND:.2f} u, U {dev_u / ssc.U_RND:.2f} u; "
          f"GPU D {got_d / ssc.U_RND:.2f} u, U {got_u / ssc.U_RND:.2f} u; allowed {allow / ssc.U_RND:.2f} u")
    assert got_d <= allow and got_u <= allow, (got_d, got_u, allow)
