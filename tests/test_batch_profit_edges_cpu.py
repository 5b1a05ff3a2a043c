"""CPU: what tests/test_gpu_batch_profit_edges.py leans on, asserted on the restatement (tests/batch_profit_reference.py) so that
no GPU comparison there can pass vacuously: the edge family reaches every path of the optim_q stop rules on both spaces, the
tie list of round() is not empty, the synthetic table reaches every outcome of the oracle's retry branch from both cursor
values, the non-finite rows run through the restatement to the outcomes the GPU tests then compare, and the two libm figures
from which the independent-answer bounds are derived are what the reference module pins."""
import math

import numpy as np
import pytest

import batch_profit_reference as ref

SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]


# ---- safe arithmetic ----------------------------------------------------------------------------------------------------------
def test_division_is_ieee():
    inf, nan = math.inf, math.nan
    cases = [(1.0, 0.0, inf), (-1.0, 0.0, -inf), (1.0, -0.0, -inf), (-2.5, -0.0, inf), (inf, 0.0, inf), (-inf, -0.0, inf),
             (1.0, inf, 0.0), (-1.0, inf, -0.0), (1.0, -inf, -0.0), (5e-324, inf, 0.0), (1e308, 1e-308, inf),
             (3.0, 7.0, 3.0 / 7.0), (1e-308, 1e308, 1e-308 / 1e308)]
    for a, b, want in cases:
        got = ref.fdiv(a, b)
        assert ref.bits(got) == ref.bits(want), (a, b, got)
    with np.errstate(all="ignore"):
        for a, b in [(0.0, 0.0), (-0.0, 0.0), (nan, 0.0), (inf, inf), (-inf, inf), (nan, 1.0), (1.0, nan)] + \
                [(a, b) for a, b, _ in cases]:
            want = float(np.float64(a) / np.float64(b))
            got = ref.fdiv(a, b)
            assert (math.isnan(got) and math.isnan(want)) or ref.bits(got) == ref.bits(want), (a, b, got, want)


def test_the_oracles_divide_by_zero_and_infinity():
    """den = gamma + vx = 0 and exp_val = inf: a gradient of +-inf or NaN, not an exception"""
    om = ref.ProfitOracle(ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V)
    vx = ref.TIE_V[0] * ref.ell_exp(1.0) + ref.TIE_V[1] * ref.ell_exp(1.0)
    (g, beta), shrunk, _ = om.assess_optim([1.0, 1.0], -vx)        # ln(0) = -inf: feasible, then q / exp_val as usual
    assert shrunk and all(math.isfinite(t) for t in g)
    (g, beta), shrunk, _ = om.assess_optim([1.0, 1.0], math.inf)   # ln(inf) - log_cobb > 0: a cut with q / inf
    assert not shrunk and beta == math.inf and g == [-ref.TIE_A[0], -ref.TIE_A[1]]
    om = ref.ProfitOracle(ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V)
    (g, beta), shrunk, gamma = om.assess_optim([-math.inf, -math.inf], 0.0)   # log_cobb = -inf, exp_val = 0, q = 0: 0 / 0
    assert shrunk and gamma == 0.0 and all(math.isnan(t) for t in g)


# ---- the edge family ----------------------------------------------------------------------------------------------------------
def test_edge_family_is_one_fixed_draw():
    params, a, v, _, xc0 = ref.edge_family()
    assert params.shape == (1500, 3) and (ref.EDGE_B, ref.EDGE_SEED) == (1500, 14)
    assert 0.5 <= params[:, 2].min() < 1.0 and params[:, 2].max() > 59.0
    assert ref.bits(float(params[0, 2])) == ref.bits(float(np.random.default_rng(14).uniform(0.5, 60.0, 4500)[3000]))
    fam = ref.family(1500, 14)
    for i in (1, 2, 4):   # the rest as in `family`
        assert np.array_equal(ref.edge_family()[i], fam[i])
    assert np.array_equal(params[:, :2], fam[0][:, :2])
    assert len(ref.EDGE_MEMBERS) <= 257 and len(set(ref.EDGE_MEMBERS)) == len(ref.EDGE_MEMBERS)


@pytest.mark.parametrize("stable", SPACES)
def test_edge_family_reaches_every_stop_rule(stable):
    tol = ref.EDGE_TOLS[0]
    recs = {b: ref.edge_solve(b, stable, tol) for b in ref.EDGE_MEMBERS}
    paths = {b: ref.edge_paths(r) for b, r in recs.items()}
    at_tol = [b for b in recs if "a" in paths[b]]
    assert len(at_tol) >= 2                                                                  # (a)
    on_noeffect = [b for b in recs if "b" in paths[b]]
    assert sorted(on_noeffect) == sorted(ref.EDGE_TOL_ON_NOEFFECT[stable]) and len(on_noeffect) >= 2   # (b)
    for b in on_noeffect:   # the run returned with retry pending: NoEffect on a first offer, status Success
        was_retry, shrunk, st = recs[b]["trace"][-1]
        assert (was_retry, st, recs[b]["status"]) == (False, ref.NOEFFECT, ref.SUCCESS)
    midrun = sorted((b, min(p[1] for p in paths[b] if isinstance(p, tuple))) for b in recs
                    if any(isinstance(p, tuple) for p in paths[b]))
    assert midrun == sorted(ref.EDGE_NOEFFECT_MIDRUN[stable]) and len(midrun) >= 2           # (c)
    for b, j in midrun:   # round j offered its first cut, which had no effect; round j + 1 is the retry
        trace = recs[b]["trace"]
        assert trace[j][0] is False and trace[j][2] == ref.NOEFFECT and trace[j + 1][0] is True
        cut = ref.edge_solve(b, stable, tol, j + 1)
        assert cut["niter"] == j + 1 and cut["status"] == ref.SUCCESS and cut["trace"] == trace[:j + 1]
    # every other end is among what is compared as well, and the looser tolerance ends everything at the tolerance
    assert {r["status"] for r in recs.values()} == {ref.SUCCESS, ref.NOSOLN, ref.NOEFFECT}
    loose = [ref.edge_solve(b, stable, ref.EDGE_TOLS[1]) for b in ref.EDGE_MEMBERS]
    assert sum("a" in ref.edge_paths(r) for r in loose) >= 100
    assert all(r["niter"] < ref.MAX_ITERS for r in loose) and len({r["niter"] for r in loose}) > 5


@pytest.mark.parametrize("stable", SPACES)
def test_a_retry_never_ends_in_success(stable):
    """Over the edge batch at both tolerances and 1e-20, and the family: a retry round repeats the cut at yd, the space has
    not moved, and the update gives NoEffect again.  So the driver's clearing of `retry` on Success after a retry round
    (batch_loop_kernels.hpp, `best || st == ST_SUCCESS`) is not reachable with this oracle: no test runs it."""
    retries = successes = shrunk = 0
    for tol in ref.EDGE_TOLS + (ref.TOL,):
        for b in ref.EDGE_MEMBERS:
            for was_retry, sh, st in ref.edge_solve(b, stable, tol)["trace"]:
                retries += was_retry
                successes += was_retry and st == ref.SUCCESS
                shrunk += was_retry and sh
    assert retries >= 6 and successes == 0
    assert all(ref.solve(ref.DISCRETE, b, stable)["status"] != ref.SUCCESS or ref.solve(ref.DISCRETE, b, stable)["retries"] == 0
               for b in range(ref.FAMILY_B))


# ---- ties and the clamp -------------------------------------------------------------------------------------------------------
def test_ties_exist():
    ties = ref.tie_list()
    print(f"{len(ties)} ties over {len({k for k, _ in ties})} values of k")
    assert len(ties) >= 10 and len({k for k, _ in ties}) >= 10
    for k, y in ties:
        assert ref.ell_exp(y) == k + 0.5 and ref.rust_round(ref.ell_exp(y)) == k + 1.0   # away from zero; rint gives the even one
        assert float(np.rint(k + 0.5)) == (k if k % 2 == 0 else k + 1)
    assert any(k % 2 == 0 for k, _ in ties)
    for y in (-0.6931471805599453, 1.252762968495368, 1.5040773967762742):
        assert y in [t for _, t in ties]
    below = float(np.nextafter(ref.ell_log(0.5), -math.inf))
    assert ref.ell_exp(below) == 0.49999999999999994 < 0.5 and ref.rust_round(ref.ell_exp(below)) == 0.0
    pts = ref.tie_points()
    assert below in pts[:, 0] and below in pts[:, 1] and len(pts) <= 514
    om = ref.ProfitOracleQ(ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V)
    _, shrunk, x_q, more, _ = om.assess_optim_q([below, below], 0.0, False)   # d = 0 -> 1, yd = ln 1 = +0.0
    assert shrunk and more and ref.bits(x_q[0]) == 0 and ref.bits(x_q[1]) == 0
    for y in pts:   # the table's problem is feasible at every point, so every call reaches round()
        om = ref.ProfitOracleQ(ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V)
        _, _, x_q, _, _ = om.assess_optim_q([float(y[0]), float(y[1])], 0.0, False)
        assert x_q[0] == ref.ell_log(max(1.0, ref.rust_round(ref.ell_exp(float(y[0]))))), y


# ---- the retry branch through the wide call -----------------------------------------------------------------------------------
def test_retry_table_reaches_every_outcome():
    params, a, v, steps = ref.retry_table()
    assert len(steps) == 5 and params.shape == (192, 3)
    first = steps[1]
    assert first["want"]["more"].all() and (first["want"]["x_q"] != first["x"]).any(axis=1).all()   # all made a yd
    for step in steps[2:4]:
        assert step["retry"].all() and not step["want"]["more"].any()
    retry = steps[2]
    assert (retry["x"] != first["x"]).any(axis=1).all()
    assert np.array_equal(retry["yd"], first["want"]["x_q"])
    kinds, signs = ref.retry_kinds(retry)
    for cursor in (0, 1):
        here = [b for b in range(len(kinds)) if retry["idx"][b] == cursor]
        assert len(here) >= 64, (cursor, len(here))
        for kind in ("cut0", "cut1", "shrunk"):
            assert sum(kinds[b] == kind for b in here) >= 1, (cursor, kind)
        assert {signs[b] for b in here} >= {-1.0, 1.0}, cursor
    # a cut from constraint 0 at yd means yd[0] > ln k: rounding took x1 past the limit
    for b, kind in enumerate(kinds):
        if kind == "cut0":
            assert retry["yd"][b, 0] > ref.ell_log(float(params[b, 2]))
    # the cursor does move in the retry calls, so the call after each shows what was stored
    assert (steps[3]["idx"] != steps[2]["idx"]).any() and (steps[4]["idx"] != steps[3]["idx"]).any()
    assert np.array_equal(steps[3]["yd"], steps[2]["yd"]) and (steps[4]["want"]["x_q"] != steps[4]["x"]).any()


def test_retry_on_a_fresh_oracle():
    """cursor -1, yd = (0, 0): the oracle is asked at x = (1, 1)"""
    om = ref.ProfitOracleQ(ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V)
    assert ref.oracle_state(om) == (-1, [0.0, 0.0])
    (g, beta), shrunk, x_q, more, gamma = om.assess_optim_q([0.7, -0.3], 0.0, True)
    assert shrunk and not more and x_q == [0.0, 0.0] and gamma == ref.ell_exp(ref.ell_log(1800.0)) - 25.0
    assert beta == (0.0 + g[0] * (0.0 - 0.7)) + g[1] * (0.0 + 0.3)


# ---- non-finite and extreme states --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("name", list(ref.KINDS))
def test_extreme_starts_run_through_the_restatement(name, stable):
    kind = ref.KINDS[name]
    for what, (x0, kappa, gamma0) in ref.EXTREME_STARTS.items():
        r = ref.run(kind, ref.family_oracle(kind, 5), ref.fresh(x0, stable, kappa), gamma0, ref.EXTREME_ITERS)
        if what in ("xc", "kappa"):      # NaN to max_iters: no comparison with a NaN ever stops the loop
            assert r["niter"] == ref.EXTREME_ITERS and r["status"] == ref.SUCCESS and math.isnan(r["gamma"])
            assert np.isnan(r["xc"]).all() and math.isnan(r["tsq"])
        elif what == "gamma_high":       # no point reaches gamma: NoSoln at round 0, nothing found
            assert r["niter"] == 0 and r["status"] == ref.NOSOLN and r["x_best"] is None and r["gamma"] == 1e300
            assert np.array_equal(r["xc"], x0)
        else:                            # ln(gamma + vx) is NaN, `fj > 0` false: the oracle shrinks from an infeasible gamma
            assert r["x_best"] is not None and math.isfinite(r["gamma"]) and r["gamma"] > 0.0


def test_extreme_calls_run_through_the_restatement():
    xs, gam = ref.extreme_calls()
    assert len(xs) <= 128
    for kind in (ref.PLAIN, ref.DISCRETE):
        oracles = [ref.make_oracle(kind, ref.TIE_PARAMS, ref.TIE_A, ref.TIE_V) for _ in xs]
        q = kind == ref.DISCRETE
        first = ref.wide_step(oracles, xs, gam, 0 if q else None)
        second = ref.wide_step(oracles, xs, first["want"]["gamma"], 1 if q else None)
        for w in (first["want"], second["want"]):
            print(kind, "NaN gradients", int(np.isnan(w["grad"]).any(axis=1).sum()), "infinite beta", int(np.isinf(w["beta"]).sum()),
                  "non-finite gamma", int((~np.isfinite(w["gamma"])).sum()), "shrunk", int(w["shrunk"].sum()))
            assert np.isnan(w["grad"]).any() and (~np.isfinite(w["gamma"])).any()
            assert w["shrunk"].any() and not w["shrunk"].all()
        assert np.isinf(first["want"]["beta"]).any()


# ---- the independent answers --------------------------------------------------------------------------------------------------
def test_closed_form_against_a_search():
    """closed_form on both branches: profit_at its point is its value, and no feasible neighbour of the point is better"""
    params, a, v, _, _ = ref.family()
    active = 0
    for b in range(0, 200, 7):
        star, (x1, x2) = ref.closed_form(params[b], a[b], v[b])
        active += x1 == float(params[b, 2])
        assert float(x1) <= params[b, 2]
        y = (math.log(float(x1)), math.log(float(x2)))
        assert abs(float(ref.profit_at(y, params[b], a[b], v[b]) - star)) <= 1e-9 * float(star)
        for d0, d1 in ((1e-3, 0.0), (-1e-3, 0.0), (0.0, 1e-3), (0.0, -1e-3), (-1e-3, 1e-3)):
            if y[0] + d0 <= math.log(params[b, 2]):   # no feasible neighbour is better
                assert ref.profit_at((y[0] + d0, y[1] + d1), params[b], a[b], v[b]) < star
    assert 0 < active < len(range(0, 200, 7))
    assert sum(float(ref.closed_form(params[b], a[b], v[b])[1][0]) == params[b, 2] for b in range(200)) == 144
    star = float(ref.closed_form(ref.PIN_PARAMS, ref.PIN_A, ref.PIN_V)[0])
    assert abs(star - 3404.760162828) < 1e-8
    best, (x1, x2) = ref.discrete_best(ref.PIN_PARAMS, ref.PIN_A, ref.PIN_V)
    assert best <= star and (x1, x2) == (30.0, 70.0)


def test_libm_figures_are_the_pinned_ones():
    """The two figures every bound of the independent-answer tests is a multiple of.  Measured with libm's exp and log over
    the family's 200 plain runs on Ell and the pin: worst |gamma - gamma*| / gamma* = 7.3808e-11, worst
    |gamma - profit_at(x_best)| = 4.8079 eps (exp_val + vx)."""
    gap, units = ref.libm_figures()
    print(f"libm: worst |gamma - gamma*| / gamma* = {gap:.4e}, worst |gamma - profit_at(x_best)| = {units:.4f} eps (exp_val + vx)")
    assert gap <= ref.LIBM_GAP <= 1.01 * gap
    assert units <= ref.LIBM_UNITS <= 1.01 * units
    params, a, v, _, _ = ref.family()
    for b in range(ref.FAMILY_B):   # the runs end below the optimum, never above it by more than their own rounding
        r = ref.solve_libm(b)
        assert r["status"] == ref.SUCCESS and r["x_best"] is not None
