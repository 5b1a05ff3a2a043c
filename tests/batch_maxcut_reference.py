"""CPU reference of the batched max-cut loops (include/ellhip_batch_maxcut.h): the reference's `MaxcutOracle`
(src/oracles/maxcut_oracle.rs:4-50) restated in numpy and `cutting_plane_optim` (src/cutting_plane.rs:286-313) over the CPU
oracle's spaces (oracle.OracleEll / oracle.OracleEllStable).  Test infrastructure, not product code.

Both folds keep the reference's order: np.cumsum adds one element after the other (np.sum and @ are pairwise or blocked
and are not used).  A skipped term is added as +0.0, which changes no bit of a fold that starts at +0.0.  Finished runs of
the test family are computed once per (s, n, kind, max_iters, tol, stable) and shared as read-only records; `run` drives
any table and space."""
import functools

import numpy as np

from oracle import oracle as O

SUCCESS, NOSOLN, NOEFFECT, UNKNOWN = 0, 1, 2, 3
KAPPA = 100.0
TOL = 1e-8
RANGES = {"mixed": (-1.0, 1.0), "pos": (0.0, 1.0)}
# (n, kind, max_iters) and niter of the members s = 0..5 on Ell and on EllStable
ROWS = (
    (16, "mixed", 2000, (48, 89, 66, 47, 24, 70), (68, 116, 80, 62, 37, 81)),
    (33, "mixed", 2000, (56, 166, 100, 150, 73, 143), (65, 234, 248, 182, 68, 143)),
    (16, "pos", 2000, (4, 5, 9, 3, 3, 4), (4, 5, 7, 3, 3, 4)),
    (33, "pos", 2000, (7, 7, 9, 9, 6, 9), (5, 6, 6, 5, 5, 5)),
)
ROW_IDS = [f"{r[0]}-{r[1]}" for r in ROWS]


def signs(xc):
    """x[i] = if xc[i] >= 0.0 { 1.0 } else { -1.0 } (:22): -0.0 gives +1, NaN gives -1"""
    return np.where(np.asarray(xc, dtype=np.float64) >= 0.0, 1.0, -1.0)


def fold(terms):
    """left fold from +0.0 along the last axis"""
    terms = np.asarray(terms, dtype=np.float64)
    zero = np.zeros(terms.shape[:-1] + (1,))
    with np.errstate(invalid="ignore", over="ignore"):   # inf - inf is NaN, as in the reference
        return np.cumsum(np.concatenate([zero, terms], axis=-1), axis=-1)[..., -1]


def assess_optim(w, xc, gamma):
    """((grad handed out, beta), shrunk, gamma, cut_value) exactly as the reference computes them (:21-49)"""
    w = np.asarray(w, dtype=np.float64)
    n = w.shape[0]
    x = signs(xc)
    masked = np.where(x[:, None] != x[None, :], w, 0.0)
    cut_value = float(fold(masked[np.triu_indices(n, 1)]))   # row-major over the upper triangle (:25-31)
    grad = fold(masked) * 2.0                                 # full rows; the diagonal never passes (:34-41)
    if cut_value > gamma:                                     # strict; NaN is false (:43)
        return (-grad, -cut_value), True, cut_value, cut_value
    return (-grad, gamma), False, gamma, cut_value


def weights(s, n, kind):
    """member s: (W symmetric with a zero diagonal, xc0)"""
    rng = np.random.default_rng(s)
    lo, hi = RANGES[kind]
    u = np.triu(rng.uniform(lo, hi, (n, n)), 1)
    return u + u.T, rng.normal(size=n)


def fresh(xc0, stable=False, kappa=KAPPA):
    return (O.OracleEllStable if stable else O.OracleEll).new_with_scalar(kappa, np.asarray(xc0, dtype=np.float64))


def space_record(space):
    return dict(mq=np.array(space.mq), xc=np.array(space.xc), kappa=space.kappa, tsq=space.tsq)


def run(w, max_iters, tol, space, gamma=-np.inf):
    """cutting_plane_optim of one instance on `space`: a record of everything the loop leaves, and the kinds of its cuts"""
    x_best, status, niter, central, deep, ties = None, SUCCESS, max_iters, 0, 0, 0
    for it in range(max_iters):
        x = np.array(space.xc)
        (g, beta), shrunk, gamma, cut_value = assess_optim(w, x, gamma)
        ties += not shrunk and cut_value == gamma   # a cut value that equals gamma is not an improvement
        if shrunk:
            x_best = x
            status = space.update_central_cut(g, beta)
            central += 1
        else:
            status = space.update_bias_cut(g, beta)
            deep += status == SUCCESS
        if status != SUCCESS or space.tsq < tol:
            niter = it
            break
    else:
        status = SUCCESS
    return dict(x_best=x_best, niter=niter, gamma=gamma, status=status, central=central, deep=deep, ties=int(ties),
                **space_record(space))


def _freeze(rec):
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def solve(s, n, kind, max_iters, tol=TOL, stable=False):
    """member s of the family from its fresh space"""
    w, xc0 = weights(s, n, kind)
    return _freeze(run(w, max_iters, tol, fresh(xc0, stable)))
