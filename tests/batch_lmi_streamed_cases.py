"""Problems, starts and CPU runs of the batched LMI loops on streamed batch handles (include/ellhip_batch_lmi_streamed.h),
shared by tests/test_batch_lmi_streamed_cpu.py and tests/test_gpu_batch_lmi_streamed.py.

The problems extend `family_b` of tests/batch_lmi_reference.py to one size per block: F_j = sym(randn(n, m_j, m_j)),
B_j = M M' + m_j I, c = randn(n), so the origin is strictly feasible.  A start is placed relative to the boundary of the
feasible set: with a unit direction d and h the distance from the origin to the boundary along d (bisection on the smallest
eigenvalue of any B_j - h sum_k d_k F_jk), the space is new_with_scalar(kf h^2, t h d).  t = 0 starts at the strictly
feasible origin, 0.98 just inside, 1.02 just outside (the factorisation fails late, on a small pivot), 1.5, 3 and 6 far
outside (it fails early); kf = 4 keeps the feasible set within reach, kf <= 0.01 with t >= 1.5 leaves it outside the
ellipsoid, so the deep cut answers NoSoln.

The CPU loop is batch_lmi_reference.optim / .feas over oracle.OracleEll / OracleEllStable; `run` records beside its results
the station of every oracle call, the row at which the factorisation stopped, and tsq after every update.  Records are
cached and read-only."""
import functools
import math

import numpy as np

import batch_lmi_reference as ref
from oracle import oracle as O

T_VALUES = (0.0, 0.98, 1.02, 1.5, 3.0, 6.0)
KF = 4.0
# (n, block sizes): the pinned shapes; 30 rounds (8 at n = 1024)
SHAPES = [(129, (64, 3)), (130, (64,)), (192, (5, 17, 64)), (1024, (64, 7))]
SHAPE_IDS = ["%d-%s" % (n, "x".join(map(str, ms))) for n, ms in SHAPES]


def rounds(n):
    return 8 if n >= 1023 else 30


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def problem(seed, n, ms):
    """-> (fs, bs, c): fs[j] [n][m_j][m_j], bs[j] [m_j][m_j], c [n].  With equal block sizes this is ref.family_b(seed, n, m, J)."""
    rng = np.random.default_rng(7000 + seed)
    fs = [ref.sym(rng.standard_normal((n, m, m))) for m in ms]
    bs = []
    for m in ms:
        mm = rng.standard_normal((m, m))
        bs.append(mm @ mm.T + m * np.eye(m))
    c = rng.standard_normal(n)
    return _freeze(*fs), _freeze(*bs), _freeze(c)[0]


def min_eig(fs, bs, x):
    return min(float(np.linalg.eigvalsh(b - np.tensordot(x, f, axes=1))[0]) for f, b in zip(fs, bs))


@functools.lru_cache(maxsize=None)
def boundary(seed, n, ms):
    """-> (d, h): a unit direction and the distance from the origin to the boundary of the feasible set along it"""
    fs, bs, _ = problem(seed, n, ms)
    d = np.random.default_rng(9000 + seed).standard_normal(n)
    d /= np.linalg.norm(d)
    lo, hi = 0.0, 1.0
    while min_eig(fs, bs, hi * d) > 0.0:
        lo, hi = hi, 2.0 * hi
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if min_eig(fs, bs, mid * d) > 0.0 else (lo, mid)
    return _freeze(d)[0], lo


def start(seed, n, ms, t, kf=KF):
    """-> (kappa, xc) of the start space"""
    d, h = boundary(seed, n, ms)
    return kf * h * h, t * h * d


def cpu_space(stable, kappa, xc):
    return (O.OracleEllStable if stable else O.OracleEll).new_with_scalar(kappa, np.array(xc))


class Traced(ref.RoundRobinLmi):
    """the round-robin oracle, with the station of every call and the row whose pivot came out <= 0 (-1: no block cut)"""

    def __init__(self, mat_f, mat_b=None, c=None):
        super().__init__(mat_f, mat_b, c)
        self.stations, self.rows = [], []

    def _note(self, station):
        self.stations.append(station)
        self.rows.append(self.blocks[station].ldlt.pos[1] - 1 if station < self.J else -1)

    def assess_optim(self, xc, gamma):
        out = super().assess_optim(xc, gamma)
        self._note(out[1])
        return out

    def assess_feas(self, xc):
        out = super().assess_feas(xc)
        self._note(self.J + 1 if out is None else out[1])
        return out


class Watched:
    """a space of the CPU oracle, with tsq after every update"""

    def __init__(self, space):
        self.space, self.trace = space, []

    xc = property(lambda self: self.space.xc)
    tsq = property(lambda self: self.space.tsq)

    def update_bias_cut(self, g, beta):
        status = self.space.update_bias_cut(g, beta)
        self.trace.append(self.space.tsq)
        return status

    def update_central_cut(self, g, beta):
        status = self.space.update_central_cut(g, beta)
        self.trace.append(self.space.tsq)
        return status


def space_record(space):
    return dict(mq=np.array(space.mq), xc=np.array(space.xc), kappa=space.kappa, tsq=space.tsq)


def run(prob, space, *, feas, max_iters, tol, gamma=math.inf, idx=-1, lmi0=False):
    """cutting_plane_feas (feas) or cutting_plane_optim of one problem on `space`, which is left as the loop leaves it.
    -> a record: x (x_best, or the feasible point; None without one), niter, gamma (optim), status, idx, the space, and the
    traces"""
    fs, bs, c = prob
    omega = Traced(fs, None if lmi0 else bs, None if feas else c)
    omega.idx = idx
    watched = Watched(space)
    if feas:
        x, niter, status = ref.feas(watched, omega, max_iters, tol)
        gamma = None
    else:
        x, niter, gamma, status = ref.optim(watched, omega, gamma, max_iters, tol)
    rec = dict(x=x, niter=niter, gamma=gamma, status=status, idx=omega.idx, stations=tuple(omega.stations),
               rows=tuple(omega.rows), tsq_trace=tuple(watched.trace), J=omega.J, **space_record(space))
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def record(stable, feas, seed, n, ms, t, kf=KF, max_iters=None, tol=0.0):
    """member (seed, t) of the family at (n, ms), from its start (cached and read-only)"""
    kappa, xc = start(seed, n, ms, t, kf)
    return run(problem(seed, n, ms), cpu_space(stable, kappa, xc), feas=feas,
               max_iters=rounds(n) if max_iters is None else max_iters, tol=tol)


def members(n):
    """the six starts of a pinned batch, over three problems: (seed, t)"""
    return tuple((i % 3, t) for i, t in enumerate(T_VALUES))


def mid_tol(stable, feas):
    """a tolerance from the middle of a run's own tsq trace (member (0, 1.5) at (129; 64, 3)): just above the value after
    the middle update, so the run ends there at the latest, by tsq < tol"""
    trace = record(stable, feas, 0, 129, (64, 3), 1.5)["tsq_trace"]
    return trace[len(trace) // 2] * (1.0 + 1e-9)


# id -> (n, ms, who, max_iters, tol); who: (seed, t[, kf]); tol None: mid_tol of the space and loop at hand.  The first four
# are the six starts at every pinned shape; "nosoln-*" put ellipsoids that miss the feasible set beside ones that reach it;
# "tol" ends by tsq < tol.
BATCHES = {sid: (n, ms, members(n), rounds(n), 0.0) for sid, (n, ms) in zip(SHAPE_IDS, SHAPES)}
BATCHES["nosoln-129"] = (129, (64, 3), ((0, 3.0, 0.01), (1, 1.5, KF), (0, 6.0, 1e-4), (2, 0.98, KF)), 30, 0.0)
BATCHES["nosoln-130"] = (130, (64,), ((0, 3.0, 0.01), (0, 1.5, 0.01), (1, 3.0, KF)), 30, 0.0)
BATCHES["tol"] = (129, (64, 3), ((0, 1.5), (2, 6.0), (1, 3.0)), 30, None)


def batch_records(bid, stable, feas):
    """-> (n, ms, who, max_iters, tol, records) of a pinned batch on one space and one loop"""
    n, ms, who, max_iters, tol = BATCHES[bid]
    tol = mid_tol(stable, feas) if tol is None else tol
    recs = [record(stable, feas, w[0], n, ms, w[1], w[2] if len(w) > 2 else KF, max_iters, tol) for w in who]
    return n, ms, who, max_iters, tol, recs


def stack(n, ms, who):
    """-> mat_f (J arrays [B][n][m][m]), mat_b (J arrays [B][m][m]), c [B][n], kappa [B], xc [B][n] of the members (seed, t[, kf])"""
    probs = [problem(w[0], n, ms) for w in who]
    starts = [start(w[0], n, ms, *w[1:]) for w in who]
    mat_f = [np.stack([p[0][j] for p in probs]) for j in range(len(ms))]
    mat_b = [np.stack([p[1][j] for p in probs]) for j in range(len(ms))]
    return (mat_f, mat_b, np.stack([p[2] for p in probs]), np.array([s[0] for s in starts]),
            np.stack([s[1] for s in starts]))
