"""Warm starts for the low-pass cutting-plane loops (CPU and GPU tests).  From EllStable / Ell::new_with_scalar(40, 0) every
oracle call of the first hundreds of rounds stops at one of the first passband rows; from new_with_scalar(KAPPA_WARM, x0) with
the x0 below the first 30 rounds walk the whole table, find feasible points, shrink gamma and end `_feas` runs at different
rounds.  `trace` steps the CPU loop by hand and names, for every oracle call, the return statement of assess_feas /
assess_optim (oracle/lowpass_oracle.c, src/oracles/lowpass_oracle.rs:58-150) that it took."""
import functools

import numpy as np

import batch_lowpass_reference as lp
import batch_stable_loop_reference as ref
from lowpass_probes import CONSTANT_SETS, lowpass_autocorr, negative_x0_probe, transition_probe
from oracle import oracle as O

KAPPA_WARM = 1e-3
LOOSE = lp.LOOSE
NEGATIVE_ALLOWED = tuple(CONSTANT_SETS["negative_passband_allowed"])

# the return statements, in the order of the source
PASS_HIGH, PASS_LOW, STOP_HIGH, STOP_NEGATIVE, TRANSITION_NEGATIVE, X0_NEGATIVE, SHRUNK, FEASIBLE = SITES = (
    "passband high", "passband low", "stopband", "non-negative scan elsewhere", "non-negative scan in the transition band",
    "x[0] < 0", "feasible and shrunk", "feasible")
MEMBERS = ("autocorr", "1.6 autocorr", "transition", "negative x0, negative allowed", "negative x0", "autocorr - 0.02 e0")


def starts(n):
    """the six (constants, x0) members, in the order of MEMBERS"""
    r = lowpass_autocorr(n)
    e0 = np.zeros(n)
    e0[0] = 1.0
    return [(LOOSE, r), (LOOSE, 1.6 * r), (LOOSE, transition_probe(n)), (NEGATIVE_ALLOWED, negative_x0_probe(n)),
            (LOOSE, negative_x0_probe(n)), (LOOSE, r - 0.02 * e0)]


def row_value(row, x):
    """Arr::dot (src/arr.rs:443-451): a left fold from 0.0"""
    return float(np.cumsum(row * x)[-1]) if len(x) else 0.0


def _steps(before, after, lo, hi):
    """rows a round-robin cursor over [lo, hi) visited between two states, given that it visited at least one"""
    return (after - before - 1) % (hi - lo) + 1


def return_site(omega, x, cut, state_before, state_after):
    """-> (site, rows visited) of one CPU oracle call.  cut: what assess_feas returned (None or (g, (b0, b1))) or what
    assess_optim returned (((g, (b0, b1)), shrunk, gamma)).  Decided from the cut's gradient, which is plus or minus one
    table row or -e0, and checked against the cursors and the value of that row."""
    sb, sa = state_before, state_after
    spec = omega.spectrum
    mdim, nwpass, nwstop = spec.shape[0], sa["nwpass"], sa["nwstop"]
    s = omega.s
    lp_sq, up_sq, sp_sq = s.lp_sq, s.up_sq, sa["sp_sq"]
    shrunk = False
    if cut is not None and len(cut) == 3:
        cut, shrunk, gamma = cut   # (assess_optim set sp_sq to the gamma it was given before the walk)
    # a band walked to its end, or not entered: the cursor is where it was, modulo the band (a new oracle's cursors stand
    # one row before their bands)
    whole_passband = (sa["idx1"] - sb["idx1"]) % nwpass == 0
    whole_stopband = (sa["idx3"] - sb["idx3"]) % (mdim - nwstop) == 0
    whole_transition = (sa["idx2"] - sb["idx2"]) % (nwstop - nwpass) == 0
    if cut is None or shrunk:
        assert whole_passband and whole_stopband and whole_transition and sa["more_alt"] == 0 and not x[0] < 0.0
        if shrunk:
            g, (b0, b1) = cut
            assert sa["kmax"] >= nwstop and np.array_equal(g, spec[sa["kmax"]]) and b0 == 0.0 and b1 == sa["fmax"] == gamma
            assert sa["fmax"] == row_value(spec[sa["kmax"]], x)
        return (SHRUNK if shrunk else FEASIBLE), mdim
    g, (b0, b1) = cut
    if b1 is None:
        assert whole_passband and whole_stopband
        if sa["more_alt"] == 0:
            assert whole_transition and x[0] < 0.0 and b0 == -x[0] and g[0] == -1.0 and not g[1:].any()
            return X0_NEGATIVE, mdim
        val = row_value(spec[sa["idx2"]], x)
        assert np.array_equal(g, -spec[sa["idx2"]]) and val < 0.0 and b0 == -val
        return TRANSITION_NEGATIVE, nwpass + (mdim - nwstop) + _steps(sb["idx2"], sa["idx2"], nwpass, nwstop)
    assert sa["more_alt"] == 1 and whole_transition
    for idx, sites in ((sa["idx1"], (PASS_HIGH, PASS_LOW)), (sa["idx3"], (STOP_HIGH, STOP_NEGATIVE))):
        if idx < 0:
            continue
        for site, sign in zip(sites, (1.0, -1.0)):
            if np.array_equal(g, sign * spec[idx]):
                val = row_value(spec[idx], x)
                if site == PASS_HIGH:
                    assert val > up_sq and (b0, b1) == (val - up_sq, val - lp_sq)
                elif site == PASS_LOW:
                    assert not val > up_sq and val < lp_sq and (b0, b1) == (-val + lp_sq, -val + up_sq)
                elif site == STOP_HIGH:
                    assert val > sp_sq and (b0, b1) == (val - sp_sq, val)
                else:
                    assert not val > sp_sq and val < 0.0 and (b0, b1) == (-val, -val + sp_sq)
                if idx == sa["idx1"]:
                    assert whole_stopband and (sa["fmax"], sa["kmax"]) == (sb["fmax"], sb["kmax"])
                    return site, _steps(sb["idx1"], sa["idx1"], 0, nwpass)
                assert whole_passband
                return site, nwpass + _steps(sb["idx3"], sa["idx3"], nwstop, mdim)
    raise AssertionError("the cut's gradient is no row the cursors point at")


def new_space(stable, kappa, x0, mq=None, use_parallel=True):
    cls = O.OracleEllStable if stable else O.OracleEll
    space = cls.new_with_scalar(kappa, x0) if mq is None else cls.new_with_matrix(kappa, mq, x0)
    if not use_parallel:
        ref.set_use_parallel_cut(space, 0) if stable else space.set_use_parallel_cut(False)
    return space


def trace(n, consts, x0, stable, rounds, *, feas=False, kappa=KAPPA_WARM, mq=None, use_parallel=True, tol=lp.TOL):
    """The CPU loop (src/cutting_plane.rs:205-227 and :286-313) stepped by hand from new_with_scalar(kappa, x0), or from
    new_with_matrix(kappa, mq, x0): update kind CENTRAL for a shrunk cut, else BIAS, as ref.Stepper has it.
    -> the record of ref.cpu_run (x_best, niter, gamma, status, state, mq, xc, kappa, tsq) with sites [per oracle call] and
    rows [visited, per call]"""
    kind = "lp_feas" if feas else "lp_optim"
    case = ref.Case(kind, [tuple(consts)], n, kappa, x0, max_iters=rounds, tol=tol)
    step = ref.Stepper(case, 0)
    omega = step.omega
    space = new_space(stable, kappa, x0, mq, use_parallel)
    gamma, x_best, status, sites, rows = case.gamma[0], None, ref.SUCCESS, [], []   # (a feas run has none: inf, as ref.cpu_run)
    niter = 0
    while niter < rounds:
        x = np.array(space.xc)
        before = omega.state()
        what, ukind, g, b0, b1, new_gamma = step.step(x, gamma)
        assert what != "error"
        if feas:
            cut = None if what == "found" else (g, (b0, b1))
        else:
            cut = ((g, (b0, b1)), what == "best", new_gamma)
        site, nrows = return_site(omega, x, cut, before, omega.state())
        assert nrows == omega.s.rows_visited, (site, nrows, omega.s.rows_visited)
        assert (ukind == ref.CENTRAL) == (site == SHRUNK)
        sites.append(site)
        rows.append(nrows)
        gamma = new_gamma
        if what in ("best", "found"):
            x_best = x
        if what == "found":
            break
        status = space.update(ukind, g, b0, b1)
        if status != ref.SUCCESS or space.tsq < tol:
            break
        niter += 1
    return dict(sites=sites, rows=rows, niter=niter, status=status, gamma=gamma, x_best=x_best, state=omega.state(),
                **ref.space_record(space))


# ---- batches for the device tests ---------------------------------------------------------------------------------------------
def warm_case(n, *, feas=False, rounds=30, members=None, use_parallel=True, pairs=None):
    """the members (default: all six) of starts(n), or the given (constants, x0) pairs, as one ref.Case from
    new_with_scalar(KAPPA_WARM, x0)"""
    pairs = starts(n) if pairs is None else pairs
    pairs = pairs if members is None else [pairs[m] for m in members]
    return ref.Case("lp_feas" if feas else "lp_optim", [c for c, _ in pairs], n, KAPPA_WARM, np.stack([x for _, x in pairs]),
                    max_iters=rounds, tol=lp.TOL, use_parallel=use_parallel)


def cpu_run(case, stable, max_iters=None, resume=None):
    """ref.cpu_run for either space: the CPU loop of every instance of a low-pass ref.Case -> the records.  resume: the
    live (omega, space, gamma) triples of an earlier call to continue from; the triples are returned beside the records."""
    max_iters = case.max_iters if max_iters is None else max_iters
    out, live = [], []
    for b in range(case.B):
        if resume is None:
            omega = O.OracleLowpass(case.n, *case.problems[b])
            mq = None if case.mq is None else case.mq[b]
            space, gamma = new_space(stable, case.kappa[b], case.xc[b], mq, case.use_parallel), case.gamma[b]
        else:
            omega, space, gamma = resume[b]
        if case.kind == "lp_optim":
            x, niter, gamma, status = omega.cutting_plane_optim(space, gamma, max_iters, case.tol)
        else:
            x, niter, status = omega.cutting_plane_feas(space, max_iters, case.tol)
        out.append(dict(x_best=None if x is None else np.array(x), niter=niter, gamma=gamma, status=status,
                        state=omega.state(), **ref.space_record(space)))
        live.append((omega, space, gamma))
    return out, live


@functools.lru_cache(maxsize=None)
def warm_records(n, stable, feas, rounds=30, members=None, use_parallel=True):
    """the finished CPU runs of warm_case, computed once and shared read-only"""
    recs, _ = cpu_run(warm_case(n, feas=feas, rounds=rounds, members=members, use_parallel=use_parallel), stable)
    for r in recs:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return recs
