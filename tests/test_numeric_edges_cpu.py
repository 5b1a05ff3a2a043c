"""CPU: what the oracle does at the edges of its input range, pinned so that test_gpu_numeric_edges.py rests on checked
relations: power-of-two rescaled cut sequences are the same run to the bit, a zero gradient gives the reference's NaN /
NoSoln outcomes, and a subnormal omega (|g| = 1e-154) keeps the state finite -- for the sequences and sizes the GPU file
uses, Ell and EllStable."""
import numpy as np
import pytest

from numeric_edges import (DIAG_EXPONENT, NOSOLN_BETA, SCALE_EXPONENTS, dense_start, diag_exponents, diag_scaled, mixed_seq,
                           oracle_run, queue_seq, scaled, state, subnormal_seq, with_zero)

# (variant, sequence, n, k, seed): the mixed sequences of the direct schedules and the queue sequences of the queued ones
SEQUENCES = [("ell", "mixed", 64, 40, 11), ("ell", "mixed", 1000, 40, 12), ("ell", "queue", 1024, 56, 13),
             ("ell", "queue", 1000, 24, 14), ("stable", "mixed", 640, 40, 15), ("stable", "queue", 640, 24, 16)]


def _new(orc, variant, n):
    return (orc.OracleEllStable if variant == "stable" else orc.OracleEll).new_with_scalar(1.0, np.zeros(n))


def _seq(orc, variant, kind, n, k, seed):
    return mixed_seq(orc, n, k, seed, stable=variant == "stable") if kind == "mixed" else queue_seq(n, k, seed)


@pytest.mark.parametrize("variant,kind,n,k,seed", SEQUENCES)
def test_rescaled_sequences_are_the_same_run_to_the_bit(orc, variant, kind, n, k, seed):
    cuts = _seq(orc, variant, kind, n, k, seed)
    o = _new(orc, variant, n)
    st, ts = oracle_run(o, cuts)
    base = state(o)
    assert np.all(np.isfinite(base[0])) and (kind == "queue") == np.all(st == 0)
    for e in SCALE_EXPONENTS:
        o2 = _new(orc, variant, n)
        st2, ts2 = oracle_run(o2, scaled(cuts, e))
        assert np.array_equal(st, st2), e
        assert np.array_equal(ts2, ts * 4.0 ** e), e
        got = state(o2)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[2] == base[2], e


def test_rescaling_breaks_down_beyond_the_exponents_used(orc):
    """The limit the GPU file stays inside: at 2^-300 the parallel cut's t0 * t1 (~ tsq^2) underflows in the reference."""
    n = 64
    cuts = mixed_seq(orc, n, 40, 11)
    o, o2 = _new(orc, "ell", n), _new(orc, "ell", n)
    st, _ = oracle_run(o, cuts)
    st2, _ = oracle_run(o2, scaled(cuts, -300))
    q, q2 = state(o)[0], state(o2)[0]
    assert not (np.array_equal(st, st2) and np.array_equal(q, q2))


@pytest.mark.parametrize("n,kind", [(64, "mixed"), (257, "mixed"), (64, "queue"), (257, "queue")])
def test_diagonally_rescaled_sequences_are_the_same_run_element_by_element(orc, n, kind):
    """From (D Q0 D, D xc0) the cuts (D^-1 g, beta) give the statuses, tsq and kappa of the unscaled run to the bit, and
    xc' = D xc, Q' = D Q D to the bit (D = diag(2^e_i), |e_i| <= 20; the cuts are built for the unscaled start)."""
    start = dense_start(n, 41 + n)
    cuts = mixed_seq(orc, n, 40, 17 + n, start=start) if kind == "mixed" else queue_seq(n, 40, 17 + n)
    o = orc.OracleEll.new_with_matrix(1.0, *start)
    st, ts = oracle_run(o, cuts)
    q, xc, kappa = state(o)
    assert np.all(np.isfinite(q)) and (kind == "queue") == np.all(st == 0) and np.any(xc != start[1])
    e = diag_exponents(n, 43 + n)
    assert e.min() <= -DIAG_EXPONENT + 3 and e.max() >= DIAG_EXPONENT - 3
    d = np.ldexp(1.0, e)
    o2 = orc.OracleEll.new_with_matrix(1.0, *dense_start(n, 41 + n, e))
    st2, ts2 = oracle_run(o2, diag_scaled(cuts, e))
    q2, xc2, kappa2 = state(o2)
    assert np.array_equal(st2, st) and np.array_equal(ts2, ts) and kappa2 == kappa
    assert np.array_equal(xc2, d * xc) and np.array_equal(q2, d[:, None] * q * d[None, :])
    # what the norm-wise check makes of it: an element of the scaled Q may sit 2^-80 below the largest one
    assert np.abs(q2).min() < 1e-12 * np.abs(q2).max()


# kind, b0, b1 of the zero-gradient cut -> (status, kappa finite)
ZERO_CUTS = {"bias0": (0, 0.0, None, 0, False), "parallel_bias": (0, 0.0, 0.5, 0, False), "q": (2, 0.0, None, 0, False),
             "central": (1, 0.0, None, 0, True), "parallel_central": (1, 0.0, 0.5, 0, True),
             "bias_nosoln": (0, NOSOLN_BETA, None, 1, True)}


@pytest.mark.parametrize("variant", ["ell", "stable"])
@pytest.mark.parametrize("cut", list(ZERO_CUTS))
def test_zero_gradient_after_three_cuts(orc, variant, cut):
    n = 64
    kind, b0, b1, want_st, kappa_finite = ZERO_CUTS[cut]
    o = _new(orc, variant, n)
    kinds, grads, c0, c1 = queue_seq(n, 3, 21)
    for i in range(3):
        assert o.update(int(kinds[i]), grads[i], c0[i], None if np.isnan(c1[i]) else c1[i]) == 0
    before = [a.copy() if isinstance(a, np.ndarray) else a for a in state(o)]
    assert o.update(kind, np.zeros(n), b0, b1) == want_st
    assert o.tsq == 0.0
    q, xc, kappa = state(o)
    if want_st == 1:                                 # NoSoln: tsq is updated, nothing else
        assert np.array_equal(q, before[0]) and np.array_equal(xc, before[1]) and kappa == before[2]
        return
    assert np.isfinite(kappa) == kappa_finite
    assert np.isnan(xc).all()
    # Ell: the whole matrix; EllStable: the packed buffer's factor and diagonal, not the scratch triangle the update rewrites
    assert int(np.isnan(q).sum()) == (n * n if variant == "ell" else n * (n + 1) // 2)
    if variant == "stable":
        assert np.isnan(np.triu(q) + np.tril(np.full((n, n), np.nan), -1)).all()
    # every later cut "succeeds" with tsq = NaN and leaves the state NaN
    for i in range(3):
        g = np.random.default_rng(i).standard_normal(n)
        assert o.update(i % 3, g, 0.0, None) == 0 and np.isnan(o.tsq)
    assert np.isnan(state(o)[1]).all() and int(np.isnan(state(o)[0]).sum()) >= n * (n + 1) // 2


def test_zero_gradient_positions_of_the_gpu_sequences_reach_the_oracle_outcomes(orc):
    """The sequences test_gpu_numeric_edges.py builds: a Success zero cut turns the state NaN for good, a NoSoln one halts a
    queue with tsq = 0 and the state of the cut before."""
    n = 1024
    cuts = queue_seq(n, 56, 31)
    for pos in (0, 5, 17, 47):
        o = _new(orc, "ell", n)
        st, ts = oracle_run(o, with_zero(cuts, [pos], "nan"))
        assert np.all(st == 0) and ts[pos] == 0.0 and np.isnan(ts[pos + 1:]).all() and np.isnan(o.kappa)
        o = _new(orc, "ell", n)
        st, ts = oracle_run(o, with_zero(cuts, [pos], "nosoln"), halt=True)
        assert np.all(st[:pos] == 0) and st[pos] == 1 and np.all(st[pos + 1:] == 3) and ts[pos] == 0.0
        assert np.all(np.isfinite(o.mq))


# (variant, n) -> (kappa, max |xc|) after the 8 central cuts of the subnormal sequence, at the sizes the GPU file runs it
SUBNORMAL_PINS = {
    ("ell", 16): (1.0318065465241995, 0.08725708064161547), ("stable", 16): (1.0318065465241995, 0.08799754761913074),
    ("ell", 64): (1.0019552725146146, 0.01413854926490829), ("stable", 64): (1.0019552725146146, 0.014072819306654953),
    ("ell", 128): (1.0004884153877398, 0.004917523702650135), ("stable", 128): (1.0004884153877398, 0.004913876361743312),
    ("ell", 640): (1.0000195314645777, 0.000574707699077574), ("stable", 640): (1.0000195314645777, 0.0005746309216037767),
    ("ell", 1000): (1.000008000036, 0.00030174529491105084), ("stable", 1000): (1.000008000036, 0.0003017333823900542),
    ("ell", 1024): (1.000007629427273, 0.00025058853752852543),
    ("stable", 1024): (1.000007629427273, 0.0002505623259712985),
    ("ell", 2048): (1.0000019073506792, 0.00011036211280173181),
    ("stable", 2048): (1.0000019073506792, 0.00011036146275257371)}


@pytest.mark.parametrize("variant,n", sorted(SUBNORMAL_PINS))
def test_subnormal_omega_stays_finite(orc, variant, n):
    cuts = subnormal_seq(n)
    o = _new(orc, variant, n)
    st, ts = oracle_run(o, cuts)
    assert np.all(st == 0)
    assert 0.0 < ts.min() and ts.max() < np.finfo(np.float64).tiny, "omega is meant to be subnormal at every cut"
    q, xc, kappa = state(o)
    assert np.isfinite(q).all() and np.isfinite(xc).all() and np.isfinite(kappa)
    kappa_want, xc_want = SUBNORMAL_PINS[(variant, n)]
    assert abs(kappa - kappa_want) <= 1e-14 * kappa_want        # (n^2 / (n^2 - 1))^8: central cuts do not see omega
    assert abs(float(np.max(np.abs(xc))) - xc_want) <= 1e-12 * xc_want


def test_one_more_decade_down_the_oracle_itself_goes_nan(orc):
    """|g| = 1e-155 at n = 64: omega ~ 1e-310 has lost too many bits, the state is NaN from the second cut on -- the
    subnormal tests stay at 1e-154."""
    n = 64
    kinds, grads, b0, b1 = subnormal_seq(n)
    o = _new(orc, "ell", n)
    oracle_run(o, (kinds, grads * 0.1, b0, b1))
    assert np.isnan(state(o)[1]).all()
