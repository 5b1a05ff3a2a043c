"""CPU reference of the batched bsearch (include/ellhip_batch_bsearch.h): the reference's `MyOracle3` (src/example3.rs) as a
family of linear feasibility oracles with a movable target, `cutting_plane_feas` (src/cutting_plane.rs:205-227),
`BSearchAdaptor::assess_bs` (:409-418) and `bsearch` (:441-466), restated in IEEE f64 with one rounding per operation over
the CPU oracle's spaces (oracle.OracleEll / oracle.OracleEllStable: `clone`, `set_xc`, `update_bias_cut`).  Test
infrastructure, not product code.

A row's fold `f = 0.0; for k: f += A[j][k] * x[k]` is taken for all J rows at once as a running sum along the rows of
A * x behind a column of +0.0 (numpy's accumulate adds one element after the other); `fold_scalar` is the same in plain
Python floats and tests/test_batch_bsearch_cpu.py holds the two together.

The seeded family (`family`) and its finished runs (`run`) are computed once and shared as read-only records."""
import functools

import numpy as np

from oracle import oracle as O

SUCCESS = 0
KAPPA = 100.0
INTERVAL = (-50.0, 50.0)
OUTER = (2000, 1e-8)
END_FEASIBLE, END_STATUS, END_TOL, END_MAX = 0, 1, 2, 3

# MyOracle3 (src/example3.rs:35-48) as a table; the last offset is never read
EX3_A = ((-1.0, 0.0), (0.0, -1.0), (1.0, 1.0), (2.0, -3.0))
EX3_C = (1.0, 2.0, 1.0, 0.0)


def fold_scalar(row, x):
    f = 0.0
    for a, v in zip(row, x):
        f += float(a) * float(v)
    return f


def ex3_expressions(x, y, target):
    """the reference's four fj, as written (:35-38)"""
    return [-x - 1.0, -y - 2.0, x + y - 1.0, 2.0 * x - 3.0 * y - target]


class LinFeas:
    """the oracle: J rows, J - 1 offsets, a cursor and a target"""

    def __init__(self, a, c):
        self.a = np.array(a, dtype=np.float64)
        self.c = np.array(c, dtype=np.float64)
        self.J, self.n = self.a.shape
        self.idx = -1
        self.target = -1e100
        self._sums = np.zeros((self.J, self.n + 1))

    def folds(self, x):
        np.multiply(self.a, np.asarray(x, dtype=np.float64), out=self._sums[:, 1:])
        return np.add.accumulate(self._sums, axis=1)[:, -1]

    def assess_feas(self, x):
        f = self.folds(x)
        for _ in range(self.J):
            self.idx += 1
            if self.idx == self.J:
                self.idx = 0
            j = self.idx
            fj = float(f[j]) - (self.target if j == self.J - 1 else float(self.c[j]))
            if fj > 0.0:
                return self.a[j], fj
        return None

    def update(self, gamma):
        self.target = gamma


def cutting_plane_feas(omega, space, max_iters, tol):
    """(x or None, niter, oracle calls, how it ended)                                       src/cutting_plane.rs:215-226"""
    for niter in range(max_iters):
        cut = omega.assess_feas(space.xc)
        if cut is None:
            return np.array(space.xc), niter, niter + 1, END_FEASIBLE
        status = space.update_bias_cut(cut[0], cut[1])
        if status != SUCCESS:
            return None, niter, niter + 1, END_STATUS
        if space.tsq < tol:
            return None, niter, niter + 1, END_TOL
    return None, max_iters, max_iters, END_MAX


def bsearch(omega, space, lower, upper, inner, outer):
    """bsearch over BSearchAdaptor(omega, space, inner).  Returns (feasible, niter, upper, rounds, ends [4], round0) where
    round0 counts the probes that were feasible before any cut."""
    assert lower <= upper
    u_orig = upper
    rounds, ends, round0 = 0, [0, 0, 0, 0], 0
    max_iters, tol = outer
    niter_out = max_iters
    for niter in range(max_iters):
        tau = (upper - lower) / 2.0
        if tau < tol:
            niter_out = niter
            break
        gamma = lower
        gamma += tau
        probe = space.clone()                                    # :410
        omega.update(gamma)                                      # :411
        x, k, calls, end = cutting_plane_feas(omega, probe, *inner)
        rounds += calls
        ends[end] += 1
        if x is not None:
            round0 += k == 0
            space.set_xc(x)                                      # :414
            upper = gamma
        else:
            lower = gamma
    return upper != u_orig, niter_out, upper, rounds, ends, round0


def space_of(stable, xc0, kappa=KAPPA, no_defer_trick=False):
    s = (O.OracleEllStable if stable else O.OracleEll).new_with_scalar(kappa, np.asarray(xc0, dtype=np.float64))
    if no_defer_trick:
        s.set_no_defer_trick(True)
    return s


def _frozen(a, dtype=np.float64):
    a = np.array(a, dtype=dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def family(seed, n):
    """member `seed` in n variables: (a [J][n], c [J], xc0 [n]) with J = 2 n + 3: rows +e_i, -e_i with offsets in (1, 3),
    two normal rows with offsets in (0.5, 2), a normal target row"""
    rng = np.random.default_rng(31000 + seed)
    a = np.zeros((2 * n + 3, n))
    for i in range(n):
        a[2 * i, i] = 1.0
        a[2 * i + 1, i] = -1.0
    c = np.zeros(2 * n + 3)
    c[:2 * n] = rng.uniform(1.0, 3.0, 2 * n)
    a[2 * n:2 * n + 2] = rng.standard_normal((2, n))
    c[2 * n:2 * n + 2] = rng.uniform(0.5, 2.0, 2)
    a[2 * n + 2] = rng.standard_normal(n)
    xc0 = np.random.default_rng(99 + seed).uniform(-0.2, 0.2, n)
    return _frozen(a), _frozen(c), _frozen(xc0)


def tables(n, B):
    """the first B members stacked: a [B][J][n], c [B][J], xc0 [B][n]"""
    ms = [family(b, n) for b in range(B)]
    return np.stack([m[0] for m in ms]), np.stack([m[1] for m in ms]), np.stack([m[2] for m in ms])


def _record(omega, space, res):
    feasible, niter, upper, rounds, ends, round0 = res
    return {"feasible": bool(feasible), "niter": niter, "upper": upper, "rounds": rounds, "ends": tuple(ends),
            "round0": round0, "idx": omega.idx, "target": omega.target, "xc": _frozen(space.xc), "mq": _frozen(space.mq),
            "kappa": space.kappa, "tsq": space.tsq}


@functools.lru_cache(maxsize=None)
def run(seed, n, stable, inner, outer=OUTER, interval=INTERVAL, no_defer_trick=False, again=None):
    """The finished run of member `seed`.  again = half-width: a second bsearch with the same objects over
    (upper - again, upper + again) around the first one's upper bound; the record is the second run's."""
    a, c, xc0 = family(seed, n)
    omega, space = LinFeas(a, c), space_of(stable, xc0, no_defer_trick=no_defer_trick)
    res = bsearch(omega, space, interval[0], interval[1], inner, outer)
    if again is not None:
        res = bsearch(omega, space, res[2] - again, res[2] + again, inner, outer)
    return _record(omega, space, res)


def runs(n, B, stable, inner, outer=OUTER, **kw):
    """the records of the first B members as arrays over the batch"""
    rs = [run(b, n, stable, inner, outer, **kw) for b in range(B)]
    return {"feasible": np.array([r["feasible"] for r in rs]), "niter": np.array([r["niter"] for r in rs], dtype=np.int64),
            "upper": np.array([r["upper"] for r in rs]), "rounds": np.array([r["rounds"] for r in rs], dtype=np.int64),
            "ends": np.array([r["ends"] for r in rs], dtype=np.int64), "round0": sum(r["round0"] for r in rs),
            "idx": np.array([r["idx"] for r in rs], dtype=np.int32), "target": np.array([r["target"] for r in rs]),
            "xc": np.stack([r["xc"] for r in rs])}


@functools.lru_cache(maxsize=None)
def pin(stable):
    """src/example3.rs:68-85 on Ell or EllStable: the record of the run"""
    omega, space = LinFeas(EX3_A, EX3_C), space_of(stable, [0.0, 0.0])
    return _record(omega, space, bsearch(omega, space, -100.0, 100.0, (2000, 1e-8), (2000, 1e-8)))
