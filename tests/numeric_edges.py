"""Cut sequences and state checks shared by the numeric-edge tests (test_numeric_edges_cpu.py pins what the oracle does with
them, test_gpu_numeric_edges.py holds every update schedule to it).

A sequence is the queue's form: (kinds int32[k], grads [k][n], beta0[k], beta1[k] with NaN = no second value).
  * rescaled: (2^e g, 2^e beta) for |e| <= 250 is the same run -- statuses, Q, xc and kappa to the bit, tsq times 4^e
    (the ellipsoid update is scale-free and every rounding of a power-of-two-scaled operand scales with it, as long as
    nothing under- or overflows; from |e| ~ 300 on the parallel cut's t0 * t1 ~ tsq^2 does);
  * a zero gradient (the reference's own degenerate cut, benches/ellipsoid.rs): omega = tsq = 0 -- a bias cut with
    beta = 0 or a q-cut "succeeds" and fills xc, Q and kappa with NaN, a central cut leaves kappa finite, beta > 0 is NoSoln;
  * |g| = 1e-154 from Q0 = I: omega ~ 1e-308, a subnormal, through which the reference stays finite;
  * diagonally rescaled: from the start (D Q0 D, D xc0), the cuts (D^-1 g, beta) with D = diag(2^e_i), |e_i| <= 20, are the
    same run ELEMENT BY ELEMENT -- statuses, tsq and kappa to the bit, xc' = D xc and Q' = D Q D to the bit: every term of
    every sum the update forms (Q g, g.Qg, v_j.g) is scaled by ONE power of two per sum, every element of Q and xc by its own.
    The per-element form of `rescaled`: it breaks on a hidden absolute constant, and on any sum that mixes elements of
    different rows or columns.
"""
import numpy as np

from util import TOL, dense_spd, mixed_cut, oracle_update, stable_tau

SCALE_EXPONENTS = (-200, 200)
SUBNORMAL_G = 1e-154
NOSOLN_BETA = 0.1
DIAG_EXPONENT = 20


def mixed_seq(orc, n, k, seed, stable=False, start=None):
    """util.mixed_cut's sequence (all six EllCalc entry points, a NoSoln cut every 8th) from kappa0 = 1, Q0 = I, xc0 = 0
    (start = (Q0, xc0): from that matrix and centre, Ell only), unit gradients, betas scaled by the tau the oracle itself
    sees before each cut."""
    if start is not None:
        o = orc.OracleEll.new_with_matrix(1.0, start[0], start[1])
    else:
        o = (orc.OracleEllStable if stable else orc.OracleEll).new_with_scalar(1.0, np.zeros(n))
    rng = np.random.default_rng(seed)
    kinds = np.zeros(k, dtype=np.int32)
    grads = np.empty((k, n))
    b0 = np.zeros(k)
    b1 = np.full(k, np.nan)
    for i in range(k):
        g = rng.standard_normal(n)
        g /= np.linalg.norm(g)
        tau = stable_tau(o, g) if stable else float(np.sqrt(max(o.kappa * (g @ (o.mq @ g)), 0.0)))
        kind, c0, c1 = mixed_cut(i, g, tau, rng)
        kinds[i], grads[i], b0[i] = kind, g, c0
        if c1 is not None:
            b1[i] = c1
        oracle_update(o, kind, g, c0, c1)
    return kinds, grads, b0, b1


def queue_seq(n, k, seed):
    """test_gpu_resident._cuts: k cuts over the six entry points with betas for tau ~ 1, no failing cut."""
    from test_gpu_resident import _cuts
    return _cuts(n, k, seed)


def scaled(cuts, e):
    s = 2.0 ** e
    kinds, grads, b0, b1 = cuts
    return kinds.copy(), grads * s, b0 * s, b1 * s


def diag_exponents(n, seed):
    """e_i of D = diag(2^e_i), |e_i| <= DIAG_EXPONENT, from a seeded generator"""
    return np.random.default_rng(seed).integers(-DIAG_EXPONENT, DIAG_EXPONENT + 1, n)


def dense_start(n, seed, e=None):
    """(Q0, xc0): util.dense_spd (dense, symmetric to the bit, g'Qg = O(1) for unit g) and a non-zero centre;
    e: (D Q0 D, D xc0), exact -- every element times its own power of two."""
    q0 = dense_spd(n, seed)
    xc0 = np.random.default_rng(seed + 1).standard_normal(n)
    if e is None:
        return q0, xc0
    d = np.ldexp(1.0, e)
    return np.ascontiguousarray(d[:, None] * q0 * d[None, :]), d * xc0


def diag_scaled(cuts, e):
    """(D^-1 g, beta): the cuts that do to (D Q D, D xc) what `cuts` do to (Q, xc)"""
    kinds, grads, b0, b1 = cuts
    return kinds.copy(), grads * np.ldexp(1.0, -np.asarray(e))[None, :], b0.copy(), b1.copy()


def with_zero(cuts, positions, outcome):
    """The sequence with a zero gradient at each position: outcome "nan" = bias cut with beta 0 (Success, the state becomes
    NaN), "central" = central cut (Success, kappa stays finite), "nosoln" = bias cut with beta > 0 (NoSoln, state kept)."""
    kinds, grads, b0, b1 = (a.copy() for a in cuts)
    for p in positions:
        grads[p] = 0.0
        kinds[p] = 1 if outcome == "central" else 0
        b0[p] = NOSOLN_BETA if outcome == "nosoln" else 0.0
        b1[p] = np.nan
    return kinds, grads, b0, b1


def subnormal_seq(n, k=8, seed=3):
    """k central cuts with |g| = 1e-154: omega = g'Qg ~ 1e-308 is subnormal from the first cut on."""
    rng = np.random.default_rng(seed)
    grads = rng.standard_normal((k, n))
    grads *= SUBNORMAL_G / np.linalg.norm(grads, axis=1)[:, None]
    return np.ones(k, dtype=np.int32), grads, np.zeros(k), np.full(k, np.nan)


def beta(b0, b1, i):
    return (float(b0[i]), None if np.isnan(b1[i]) else float(b1[i]))


def oracle_run(o, cuts, halt=False):
    """Statuses and tsq after every cut.  halt: the queue's contract -- after the first non-Success cut every later one
    reports Unknown (3) and leaves tsq alone (NaN here: not compared)."""
    kinds, grads, b0, b1 = cuts
    k = len(kinds)
    st = np.full(k, 3, dtype=np.int32)
    ts = np.full(k, np.nan)
    for i in range(k):
        c0, c1 = beta(b0, b1, i)
        st[i] = oracle_update(o, int(kinds[i]), grads[i], c0, c1)
        ts[i] = o.tsq
        if halt and st[i] != 0:
            break
    return st, ts


def state(space):
    """(Q, xc, kappa) of a GPU handle or an oracle"""
    xc = space.xc() if callable(space.xc) else np.array(space.xc)
    return np.array(space.mq), xc, float(space.kappa)


def assert_close_with_nans(got, want, tol=TOL, what=""):
    """Same NaN (and inf) positions; the finite entries within tol relative to the largest finite |want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN masks differ ({np.isnan(got).sum()} vs {np.isnan(want).sum()})"
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), f"{what}: infinities differ"
    if fin.any():
        assert np.all(np.isfinite(got[fin])), f"{what}: non-finite where the oracle is finite"
        scale = float(np.max(np.abs(want[fin])))
        err = float(np.max(np.abs(got[fin] - want[fin])))
        assert err <= tol * scale + 1e-300, f"{what}: abs err {err} vs scale {scale} (tol {tol})"


def assert_state_with_nans(got, want, tol=TOL, what=""):
    for name, a, b in zip(("Q", "xc", "kappa"), got, want):
        assert_close_with_nans(a, b, tol, f"{what} {name}")
