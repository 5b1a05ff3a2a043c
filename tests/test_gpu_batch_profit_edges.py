"""GPU: the profit oracles and the optim_q driver off the seeded family's road (tests/test_gpu_batch_profit.py walks that one).
The discrete kind's stop rules at tolerances that end loops on Success and on NoEffect rounds; a retry flag left in HBM by a
finished run or by a wide call; the oracle's retry branch through the wide call from synthetic states; exact ties of round()
and the zero clamp; the robust kind's sign select at +-0 and +-5e-324; non-finite and extreme arguments and starts, alone and
among 64 ordinary neighbours; the wide kernel across its 128-problem workgroups.  Those comparisons are EXACT (float64 bit
patterns, NaN by position, integers) against tests/batch_profit_reference.py, and tests/test_batch_profit_edges_cpu.py asserts
that the reference side takes every path named here.  The last section compares the device with answers that do not come from
the restatement: the closed form under mpmath, the objective at x_best, and the best integer point by brute force."""
import math

import numpy as np
import pytest

import batch_maxcut_checks as chk
import batch_profit_reference as ref

pytestmark = pytest.mark.gpu

SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]
KINDS = [pytest.param(k, id=name) for name, k in ref.KINDS.items()]
EPS = 2.0 ** -52


def space_class(gpu, stable):
    return gpu.EllStableBatch if stable else gpu.EllBatch


def edge_problem(gpu, members):
    params, a, v, _, _ = ref.edge_family()
    idx = list(members)
    return gpu.BatchProfitProblem(ref.DISCRETE, params[idx], a[idx], v[idx])


def edge_spaces(gpu, stable, members):
    idx = list(members)
    return space_class(gpu, stable).new_with_scalar(np.full(len(idx), ref.KAPPA), ref.edge_family()[4][idx])


def check_run(got, batch, recs):
    chk.assert_runs_equal(got, recs, 2)
    chk.assert_state_equal(batch, recs)


def check_wide(prob, step, what):
    """one wide call with the step's arguments against what the CPU oracles returned for them"""
    w = step["want"]
    if step["retry"] is None:
        grad, beta, shrunk, gamma = prob.assess_optim(step["x"], step["gamma"])
    else:
        grad, beta, shrunk, x_q, more, gamma = prob.assess_optim_q(step["x"], step["gamma"], step["retry"])
        chk.assert_bits(x_q, w["x_q"], (what, "x_q"))
        np.testing.assert_array_equal(more, w["more"], err_msg=str(what))
    chk.assert_bits(grad, w["grad"], (what, "grad"))
    chk.assert_bits(beta, w["beta"], (what, "beta"))
    chk.assert_bits(gamma, w["gamma"], (what, "gamma"))
    np.testing.assert_array_equal(shrunk, w["shrunk"], err_msg=str(what))


# ---- the discrete kind's stop rules -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [256, 1])
@pytest.mark.parametrize("tol", ref.EDGE_TOLS)
@pytest.mark.parametrize("stable", SPACES)
def test_stop_rules_at_a_reachable_tolerance(gpu, stable, tol, chunk):
    """ends at the tolerance on Success rounds and on NoEffect rounds, NoSoln, NoEffect after a retry; with chunk = 1 the
    flag crosses a launch after every round"""
    members = ref.EDGE_MEMBERS
    recs = [ref.edge_solve(b, stable, tol) for b in members]
    prob, batch = edge_problem(gpu, members), edge_spaces(gpu, stable, members)
    prob.set_chunk(chunk)
    check_run(prob.optim_q(batch, 0.0, ref.MAX_ITERS, tol), batch, recs)


# ---- a retry flag left behind -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES)
def test_a_run_that_ended_with_retry_pending_does_not_leak_it(gpu, stable):
    """The members of path (b) return with retry = 1 in HBM.  A second call on the same handles is a new run: retry starts
    false (src/cutting_plane.rs:343), as in the reference continued with the same oracle objects."""
    members, tol = ref.EDGE_MEMBERS, ref.EDGE_TOLS[0]
    oracles = [ref.edge_oracle(b) for b in members]
    cpu = [ref.edge_space(b, stable) for b in members]
    first = [ref.run_optim_q(oracles[i], cpu[i], 0.0, ref.MAX_ITERS, tol) for i in range(len(members))]
    prob, batch = edge_problem(gpu, members), edge_spaces(gpu, stable, members)
    got = prob.optim_q(batch, 0.0, ref.MAX_ITERS, tol)
    check_run(got, batch, first)
    second = [ref.run_optim_q(oracles[i], cpu[i], first[i]["gamma"], ref.MAX_ITERS, ref.TOL) for i in range(len(members))]
    for b in ref.EDGE_TOL_ON_NOEFFECT[stable]:   # a stale flag would make round 0 a retry: NoEffect without more_alt, niter 0
        r = second[members.index(b)]
        assert (r["niter"], r["status"]) != (0, ref.NOEFFECT), b
    check_run(prob.optim_q(batch, got[3], ref.MAX_ITERS, ref.TOL), batch, second)


@pytest.mark.parametrize("stable", SPACES)
def test_max_iters_with_a_retry_pending(gpu, stable):
    """path (c), one problem per call: max_iters = j + 1 ends the run on the NoEffect round j with the retry still to come;
    the next call starts a new run"""
    tol = ref.EDGE_TOLS[0]
    for b, j in ref.EDGE_NOEFFECT_MIDRUN[stable]:
        omega, space = ref.edge_oracle(b), ref.edge_space(b, stable)
        first = ref.run_optim_q(omega, space, 0.0, j + 1, tol)
        assert first["niter"] == j + 1
        prob, batch = edge_problem(gpu, [b]), edge_spaces(gpu, stable, [b])
        got = prob.optim_q(batch, 0.0, j + 1, tol)
        check_run(got, batch, [first])
        second = ref.run_optim_q(omega, space, first["gamma"], ref.MAX_ITERS, ref.TOL)
        check_run(prob.optim_q(batch, got[3], ref.MAX_ITERS, ref.TOL), batch, [second])


@pytest.mark.parametrize("stable", SPACES)
def test_the_wide_calls_retry_flags_do_not_reach_a_loop(gpu, stable):
    """assess_optim_q keeps the caller's flags where the driver keeps its own.  One wide call with retry = 1 everywhere, then
    a loop on fresh spaces: the loop equals the reference's from the oracle state that one call left (cursor and yd)."""
    members, tol = ref.EDGE_MEMBERS, ref.EDGE_TOLS[0]
    oracles = [ref.edge_oracle(b) for b in members]
    xc0 = ref.edge_family()[4][list(members)]
    step = ref.wide_step(oracles, xc0 + 0.25, 0.0, 1)
    prob = edge_problem(gpu, members)
    check_wide(prob, step, "retry = 1 on fresh handles")
    recs = [ref.run_optim_q(oracles[i], ref.edge_space(b, stable), 0.0, ref.MAX_ITERS, tol) for i, b in enumerate(members)]
    batch = edge_spaces(gpu, stable, members)
    check_run(prob.optim_q(batch, 0.0, ref.MAX_ITERS, tol), batch, recs)


# ---- the oracle's retry branch through the wide call --------------------------------------------------------------------------
def test_retry_branch_from_synthetic_states(gpu):
    """tests/batch_profit_reference.py: retry_table -- from both cursor values, feasibility cuts at yd from either
    constraint, shrunk cuts, both signs of beta's shift term; the call after each shows the cursor and yd it stored"""
    params, a, v, steps = ref.retry_table()
    prob = gpu.BatchProfitProblem(ref.DISCRETE, params, a, v)
    for i, step in enumerate(steps):
        check_wide(prob, step, f"call {i}")


def test_retry_on_fresh_handles(gpu):
    """cursor -1, yd = (0, 0), then a second retry and an ordinary call"""
    B = 5
    oracles = [ref.make_oracle(ref.DISCRETE, ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V) for _ in range(B)]
    prob = gpu.BatchProfitProblem(ref.DISCRETE, np.tile(ref.TIE_PARAMS, (B, 1)), np.tile(ref.TIE_A, (B, 1)),
                                  np.tile(ref.TIE_V, (B, 1)))
    x = np.array([[0.7, -0.3], [-1.0, 2.0], [3.0, 3.0], [0.0, 0.0], [5.0, -2.0]])
    gamma = np.array([0.0, 100.0, 1e5, 1774.0, -20.0])
    for i, retry in enumerate((1, 1, 0, 1)):
        step = ref.wide_step(oracles, x + 0.125 * i, gamma, retry)
        check_wide(prob, step, f"call {i}")
        gamma = step["want"]["gamma"]


# ---- ties of round() and the zero clamp ---------------------------------------------------------------------------------------
def tie_chunks():
    pts = ref.tie_points()
    return [pts[i:i + 257] for i in range(0, len(pts), 257)]


def tie_problem(gpu, kind, B):
    return gpu.BatchProfitProblem(kind, np.tile(ref.TIE_PARAMS, (B, 1)), np.tile(ref.TIE_A, (B, 1)), np.tile(ref.TIE_V, (B, 1)))


def test_ties_and_the_clamp_in_wide_calls(gpu):
    """ell_exp(y) = k + 0.5 exactly: round goes away from zero (rint would take the even neighbour); just below ln 0.5 the
    rounded value is 0, clamped to 1, and yd = +0.0.  x_q shows which way each went."""
    for pts in tie_chunks():
        B = len(pts)
        oracles = [ref.make_oracle(ref.DISCRETE, ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V) for _ in range(B)]
        prob = tie_problem(gpu, ref.DISCRETE, B)
        first = ref.wide_step(oracles, pts, 0.0, 0)
        assert first["want"]["shrunk"].all()
        check_wide(prob, first, "at the ties")
        check_wide(prob, ref.wide_step(oracles, pts[::-1], first["want"]["gamma"] - 1.0, 0), "at the ties, reversed")


@pytest.mark.parametrize("stable", SPACES)
def test_ties_and_the_clamp_in_short_loops(gpu, stable):
    for pts in tie_chunks():
        B = len(pts)
        recs = [ref.run_optim_q(ref.make_oracle(ref.DISCRETE, ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V),
                                ref.fresh(pts[b], stable), 0.0, 4, ref.TOL) for b in range(B)]
        assert all(r["x_best"] is not None for r in recs)
        prob = tie_problem(gpu, ref.DISCRETE, B)
        batch = space_class(gpu, stable).new_with_scalar(np.full(B, ref.KAPPA), pts)
        check_run(prob.optim_q(batch, 0.0, 4, ref.TOL), batch, recs)


# ---- the robust kind's sign select --------------------------------------------------------------------------------------------
def test_robust_sign_select_at_the_zeros(gpu):
    """`y[i] > 0.0`: false at +0.0, -0.0 and -5e-324, true at 5e-324; all 16 pairs, two calls each"""
    vals = [0.0, -0.0, 5e-324, -5e-324]
    x = np.array([(p, q) for p in vals for q in vals])
    B = len(x)
    params, a, v, vparams, _ = ref.family()
    oracles = [ref.family_oracle(ref.ROBUST, b) for b in range(B)]
    prob = gpu.BatchProfitProblem(ref.ROBUST, params[:B], a[:B], v[:B], vparams[:B])
    first = ref.wide_step(oracles, x, 0.0)
    for b in range(B):   # the select shows in the cut: the same problem asked at (+0, +0) gives another gradient
        if 5e-324 in x[b]:
            at_zero = ref.family_oracle(ref.ROBUST, b).assess_optim([0.0, 0.0], 0.0)[0][0]
            assert not chk.same_bits(first["want"]["grad"][b], at_zero), b
    check_wide(prob, first, "first call")
    check_wide(prob, ref.wide_step(oracles, x[::-1], first["want"]["gamma"]), "second call")


# ---- non-finite and extreme arguments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [pytest.param(ref.PLAIN, id="plain"), pytest.param(ref.DISCRETE, id="discrete")])
def test_extreme_arguments_in_wide_calls(gpu, kind):
    """y at and past the ends of exp's range, +-inf and NaN; gamma = -vx exactly (ln 0), below it (ln of a negative), +inf,
    1e308 and NaN.  The second call is a retry in the discrete kind, from whatever yd the first one made."""
    xs, gam = ref.extreme_calls()
    q = kind == ref.DISCRETE
    oracles = [ref.make_oracle(kind, ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V) for _ in xs]
    prob = tie_problem(gpu, kind, len(xs))
    first = ref.wide_step(oracles, xs, gam, 0 if q else None)
    check_wide(prob, first, "first call")
    check_wide(prob, ref.wide_step(oracles, xs, first["want"]["gamma"], 1 if q else None), "second call")


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("kind", KINDS)
def test_extreme_starts_among_ordinary_neighbours(gpu, kind, stable):
    """B = 65: a workgroup of 64 family members and one more.  One member at a time starts from xc0 = (-800, 720), from
    kappa = 1e300, from gamma0 = 1e300 or from gamma0 = -1e9, at position 0, 31 or 63; its record and its 64 neighbours'
    equal the CPU's, so a NaN in one problem's lanes reaches no other problem."""
    B, iters = 65, ref.EXTREME_ITERS
    params, a, v, vparams, xc0 = ref.family()
    usual = [ref.solve(kind, b, stable, iters) for b in range(B)]
    prob = gpu.BatchProfitProblem(kind, params[:B], a[:B], v[:B], vparams[:B] if kind == ref.ROBUST else None)
    for what, (x0, kappa0, gamma0) in ref.EXTREME_STARTS.items():
        for pos in (0, 31, 63):
            start, kappa, gamma = np.array(xc0[:B]), np.full(B, ref.KAPPA), np.zeros(B)
            start[pos], kappa[pos], gamma[pos] = x0, kappa0, gamma0
            recs = list(usual)
            recs[pos] = ref.run(kind, ref.family_oracle(kind, pos), ref.fresh(x0, stable, kappa0), gamma0, iters)
            batch = space_class(gpu, stable).new_with_scalar(kappa, start)
            got = (prob.optim_q if kind == ref.DISCRETE else prob.optim)(batch, gamma, iters, ref.TOL)
            chk.assert_runs_equal(got, recs, 2)
            chk.assert_state_equal(batch, recs)
            # the handle's cursors and yd went through these runs: a fresh handle for the next start
            prob = gpu.BatchProfitProblem(kind, params[:B], a[:B], v[:B], vparams[:B] if kind == ref.ROBUST else None)


# ---- the wide kernel's workgroups ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [128, 129, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_wide_kernel_shapes(gpu, kind, B):
    """k_batch_profit_assess holds 128 problems per workgroup: one full, one full and a single problem, two full and one"""
    params, a, v, vparams, xc0 = ref.family(B)
    q = kind == ref.DISCRETE
    oracles = [ref.make_oracle(kind, tuple(params[b]), a[b], v[b], tuple(vparams[b])) for b in range(B)]
    prob = gpu.BatchProfitProblem(kind, params, a, v, vparams if kind == ref.ROBUST else None)
    first = ref.wide_step(oracles, xc0, 0.0, 0 if q else None)
    check_wide(prob, first, "first call")
    second = ref.wide_step(oracles, xc0 - 0.5, first["want"]["gamma"], np.arange(B) % 2 if q else None)
    check_wide(prob, second, "second call")
    check_wide(prob, ref.wide_step(oracles, xc0 - 0.25, second["want"]["gamma"], 0 if q else None), "third call")


# ---- independent answers ------------------------------------------------------------------------------------------------------
# Bounds: multiples of the two figures measured on the libm reference runs (ref.LIBM_GAP, ref.LIBM_UNITS), the
# factor 4 because an ell_exp / ell_log run takes another iteration path than libm's.  Nothing below compares the device
# with itself or with the restatement's runs.
def family_problem(gpu, kind, stable):
    params, a, v, vparams, xc0 = ref.family()
    prob = gpu.BatchProfitProblem(kind, params, a, v, vparams if kind == ref.ROBUST else None)
    batch = space_class(gpu, stable).new_with_scalar(np.full(ref.FAMILY_B, ref.KAPPA), xc0)
    x_best, has, niter, gamma, status = (prob.optim_q if kind == ref.DISCRETE else prob.optim)(batch, 0.0, ref.MAX_ITERS, ref.TOL)
    assert has.all()
    return x_best, gamma


def pin_problem(gpu, kind):
    vp = np.array([ref.PIN_VPARAMS]) if kind == ref.ROBUST else None
    prob = gpu.BatchProfitProblem(kind, np.array([ref.PIN_PARAMS]), np.array([ref.PIN_A]), np.array([ref.PIN_V]), vp)
    batch = gpu.EllBatch.new(np.full((1, 2), 100.0), np.zeros((1, 2)))
    x_best, has, niter, gamma, status = (prob.optim_q if kind == ref.DISCRETE else prob.optim)(batch, 0.0, ref.MAX_ITERS, ref.TOL)
    assert has.all()
    return x_best, gamma


def cases_of(gpu, kind, stable):
    """(x_best, gamma, params, a, v) of the family's 200 and the pin"""
    params, a, v, _, _ = ref.family()
    x_best, gamma = family_problem(gpu, kind, stable)
    out = [(x_best[b], float(gamma[b]), params[b], a[b], v[b]) for b in range(ref.FAMILY_B)]
    x_best, gamma = pin_problem(gpu, kind)
    return out + [(x_best[0], float(gamma[0]), np.array(ref.PIN_PARAMS), np.array(ref.PIN_A), np.array(ref.PIN_V))]


@pytest.mark.parametrize("stable", SPACES)
def test_plain_gamma_is_the_optimum(gpu, stable):
    worst_gap = worst_units = 0.0
    for x_best, gamma, p, a, v in cases_of(gpu, ref.PLAIN, stable):
        star = ref.closed_form(p, a, v)[0]
        revenue, cost = ref.profit_terms(x_best, p, a, v)
        gap = float(abs(gamma - star) / star)
        units = ref.eps_units(gamma, x_best, p, a, v)
        worst_gap, worst_units = max(worst_gap, gap), max(worst_units, units)
        assert gap <= 4.0 * ref.LIBM_GAP, (gap, p)
        assert float(gamma - star) <= ref.LIBM_UNITS * EPS * float(revenue + cost), (gamma, float(star), p)
        assert x_best[0] <= ref.ell_log(float(p[2])), (x_best, p)   # feasible: x1 <= k
        assert units <= 4.0 * ref.LIBM_UNITS, (units, p)
    print(f"plain: worst |gamma - gamma*| / gamma* = {worst_gap:.3e}, worst |gamma - profit_at(x_best)| = {worst_units:.2f} eps units")


@pytest.mark.parametrize("stable", SPACES)
def test_robust_gamma_is_below_the_nominal_optimum(gpu, stable):
    """every shift tightens the problem: p - e3, k - e4, v + e5, and a -+ uie by the side that lowers the revenue"""
    for x_best, gamma, p, a, v in cases_of(gpu, ref.ROBUST, stable):
        assert 0.0 < gamma <= float(ref.closed_form(p, a, v)[0]), (gamma, p)


@pytest.mark.parametrize("stable", SPACES)
def test_discrete_answer_is_an_integer_point(gpu, stable):
    worst = 0.0
    for x_best, gamma, p, a, v in cases_of(gpu, ref.DISCRETE, stable):
        ints = [float(np.rint(math.exp(x_best[0]))), float(np.rint(math.exp(x_best[1])))]
        assert chk.same_bits(x_best, [ref.ell_log(ints[0]), ref.ell_log(ints[1])]), (x_best, ints)   # an integer point
        assert 1.0 <= ints[0] <= p[2] and ints[1] >= 1.0, (ints, p)                                    # x1 <= k
        revenue, cost = ref.profit_terms(x_best, p, a, v)
        bound = 4.0 * ref.LIBM_UNITS * EPS * float(revenue + cost)
        worst = max(worst, ref.eps_units(gamma, x_best, p, a, v))
        assert abs(float(gamma - ref.profit_at(x_best, p, a, v))) <= bound, (gamma, p)
        assert gamma <= ref.discrete_best(p, a, v)[0] + bound, (gamma, ref.discrete_best(p, a, v), p)
    print(f"discrete: worst |gamma - profit_at(x_best)| = {worst:.2f} eps units")
