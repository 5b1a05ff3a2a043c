"""Builders and checkers for the LMI oracle tests: plain numpy, no GPU, no oracle import.

Two families of inputs whose failing pivot is known WITHOUT an O(m^3) factorisation on the host, and checkers that
judge what a factorisation returned (`storage`, `pos`, `wit`, ep, g) against the input alone.

Notation: S is LDLTMgr::storage (src/oracles/ldlt_mgr.rs): strict lower triangle L, diagonal D, strict upper
triangle T[k][j] = L[j][k] * D[k] ("keep for later").  p is pos.1 (failing row + 1), or the order m for an SPD
matrix.  u = 2^-53.

How the checkers evaluate their own side.  Up to order LONGDOUBLE_MAX_P they accumulate in np.longdouble (64-bit
significand: their own error is 2^-11 of the bound), in row blocks, never an m x m longdouble array.  Above it (and on
a platform whose long double is only a double) they accumulate in float64 and DOUBLE the bound: a float64 sum of
products, in any order, is off from the exact value by at most gamma_p = p u / (1 - p u) times the sum of the
products' magnitudes -- the very same nonnegative sum the bound is made of -- so `device error + checker error`
stays under twice the bound whenever the device is inside the bound.  That is exact for the single-product checks
(witness, ep, quad); the probe nests three products and its float64 worst case is larger than one gamma_p, but a
failure there can only be a false alarm, never a missed error, and the reference sits at 1e-2 of the bound.  The
bounds themselves are sums of nonnegative terms, evaluated in float64 (relative error p u: immaterial).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_MAX_P = 2100
_BLOCK = 256
_EXTENDED = np.finfo(np.longdouble).eps < 2.0 ** -60


def _acc(p):
    """(accumulation dtype, factor on the bound) for a check of order p"""
    if _EXTENDED and p <= LONGDOUBLE_MAX_P:
        return np.longdouble, 1.0
    return np.float64, 2.0


# ---------------------------------------------------------------------------------------------------- builders

class ExactPencil:
    """A[i][j] = c[min(i, j)] s_i s_j with c = cumsum(D), D_k in {0.5, 1, 2, 4}, s_i = +-2^e, e in [-3, 3].

    Its LDL^T is L[i][j] = s_i / s_j, diagonal D_k s_k^2, T[k][j] = s_j s_k D_k, and every intermediate of the
    factorisation (the partial sums s_i s_j c[k], the quotients, the pivots) is exactly representable in fp64:
    whatever order a correct implementation sums in, it must return these very bits.

    The SPD matrix and its factor are built once; `case(pivot, value)` replaces D_pivot by `value` (0.0, or a tiny
    negative number), which moves only A[pivot:, pivot:] and the one diagonal entry of the factor the reference
    still writes before it stops."""

    def __init__(self, m, rng):
        self.m = int(m)
        self.D = rng.choice(np.array([0.5, 1.0, 2.0, 4.0]), size=self.m)
        self.s = rng.choice(np.array([-1.0, 1.0]), size=self.m) * 2.0 ** rng.integers(-3, 4, size=self.m)
        self.c = np.cumsum(self.D)  # multiples of 0.5 below 2^16: exact
        idx = np.arange(self.m, dtype=np.int32)
        self.A = self.c[np.minimum.outer(idx, idx)]
        self.A *= self.s[:, None]
        self.A *= self.s[None, :]
        self.S = np.tril(np.outer(self.s, 1.0 / self.s), -1)
        self.S += np.triu(np.outer(self.D * self.s, self.s))

    def case(self, pivot=None, value=0.0):
        """(A, expected storage[:rows, :rows], pos, ep); ep is None for the SPD case.  The arrays of the SPD case
        are the shared ones: do not write to them."""
        if pivot is None:
            return self.A, self.S, (0, 0), None
        k, value = int(pivot), float(value)
        assert 0 <= k < self.m and value <= 0.0
        before = float(self.c[k - 1]) if k else 0.0
        ck = before + value
        if Fraction(ck) != Fraction(before) + Fraction(value):
            raise ValueError(f"c[{k}] = {before!r} + {value!r} is not representable in fp64: the factor would not be exact")
        c = self.c.copy()
        c[k:] += value - self.D[k]  # rows past k are never read back; only c[k] has to be exact
        c[k] = ck
        A = self.A.copy()
        idx = np.arange(k, self.m, dtype=np.int32)
        A[k:, k:] = c[np.minimum.outer(idx, idx)] * self.s[k:, None] * self.s[None, k:]
        S = self.S[:k + 1, :k + 1].copy()
        S[k, k] = value * self.s[k] ** 2
        return A, S, (0, k + 1), -S[k, k]


def exact_pencil(m, rng, pivot=None, value=0.0):
    """One case of a fresh ExactPencil: (A, expected storage[:rows, :rows], pos, ep)."""
    return ExactPencil(m, rng).case(pivot, value)


def generic_pencil(m, p, rng, r=8):
    """U U' + diag(d), d in [1, 2), U m x r, then entry [p-1][p-1] = -1.0.  The matrix before that last step is
    >= I, so every leading Schur complement before row p-1 is >= 1, and the one at row p-1 is <= -1 (a Schur
    complement never exceeds the entry it starts from): pos == (0, p), with margins no rounding can cross."""
    u = rng.standard_normal((m, r))
    a = u @ u.T
    for r0 in range(0, m, 512):  # bitwise symmetric, whatever the GEMM did: the lower triangle is the matrix
        for c0 in range(0, r0 + 1, 512):
            a[c0:c0 + 512, r0:r0 + 512] = a[r0:r0 + 512, c0:c0 + 512].T
    a[np.arange(m), np.arange(m)] += 1.0 + rng.random(m)
    a[p - 1, p - 1] = -1.0
    return a


def second_matrix(m, rng):
    """A dense symmetric F_1 = a b' + b a' to ride along with x_1 = 0.0 (F(x) is unchanged: s + F_1[i][j] * 0.0 == s).
    With F_0 = F(x) itself, v'F_0 v collapses to the failing pivot: A v = D_p e_p on the leading block, so every
    row chunk of k_lmi_quad but the last sums to rounding noise and a lost chunk would go unseen.  Every row of
    F_1 carries weight in v'F_1 v."""
    a, b = rng.standard_normal(m), rng.standard_normal(m)
    f = np.outer(a, b)
    f += np.outer(b, a)  # a_i b_j + b_i a_j: symmetric bit for bit, addition commutes
    return f


# ---------------------------------------------------------------------------------------------------- checkers

def _l_blocks(S, p, dtype):
    """(r0, r1, rows r0:r1 of the unit lower L, columns [:r1]) over the leading p x p block"""
    for r0 in range(0, p, _BLOCK):
        r1 = min(p, r0 + _BLOCK)
        lb = S[r0:r1, :r1].astype(dtype)
        lb[:, r0:r1] = np.tril(lb[:, r0:r1], -1) + np.eye(r1 - r0, dtype=dtype)
        yield r0, r1, lb


def _lt_mul(S, p, x, dtype):
    """L' x for x of shape (p, nx)"""
    out = np.zeros(x.shape, dtype=dtype)
    for r0, r1, lb in _l_blocks(S, p, dtype):
        out[:r1] += lb.T @ x[r0:r1].astype(dtype)
    return out


def _l_mul(S, p, x, dtype):
    """L x"""
    out = np.zeros(x.shape, dtype=dtype)
    for r0, r1, lb in _l_blocks(S, p, dtype):
        out[r0:r1] = lb @ x[:r1].astype(dtype)
    return out


def _abs_lt_mul(S, p, x):
    out = np.zeros(x.shape)
    for r0, r1, lb in _l_blocks(S, p, np.float64):
        out[:r1] += np.abs(lb).T @ x[r0:r1]
    return out


def _abs_l_mul(S, p, x):
    out = np.zeros(x.shape)
    for r0, r1, lb in _l_blocks(S, p, np.float64):
        out[r0:r1] = np.abs(lb) @ x[:r1]
    return out


def _worst_ratio(res, bound):
    """max |res| / bound, with 0 / 0 = 0 and x / 0 = inf"""
    res, bound = np.abs(np.asarray(res, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
    ratio = np.where(bound > 0.0, res / np.where(bound > 0.0, bound, 1.0), np.where(res == 0.0, 0.0, np.inf))
    return float(np.max(ratio))


def _quad(M, v, p, dtype):
    """(v' M v, sum |v_i M_ij v_j|) over the leading p x p block"""
    vv = v[:p].astype(dtype)
    va = np.abs(v[:p])
    val, mag = dtype(0.0), 0.0
    for r0 in range(0, p, _BLOCK):
        r1 = min(p, r0 + _BLOCK)
        val += vv[r0:r1] @ (M[r0:r1, :p].astype(dtype) @ vv)
        mag += float(va[r0:r1] @ (np.abs(M[r0:r1, :p]) @ va))
    return val, mag


def check_witness(S, v, p):
    """wit solves L' v = e_p on the leading block: v[p-1] == 1, v[p:] == 0, |L'v - e_p| <= p u |L|'|v| column by
    column (each v_c is one inner product of at most p terms).  Returns the worst residual / bound."""
    assert v[p - 1] == 1.0, v[p - 1]
    assert not np.any(v[p:]), "witness is not zero past the failing row"
    dtype, f = _acc(p)
    res = _lt_mul(S, p, v[:p, None], dtype)[:, 0]
    res[p - 1] -= 1.0
    bound = f * p * U * _abs_lt_mul(S, p, np.abs(v[:p, None]))[:, 0]
    ratio = _worst_ratio(res, bound)
    assert ratio <= 1.0, f"witness residual is {ratio:.3g} x its bound (p = {p})"
    return ratio


def check_factor_probe(A, S, p, z):
    """|A z - L (D (L' z))| <= p u |L| (|D| (|L|' |z|)) componentwise on the leading p x p block, for the probe
    vectors z of shape (p,) or (p, nz): the LDL' backward error bound, seen through z.  Returns the worst ratio."""
    z = np.asarray(z, dtype=np.float64).reshape(p, -1)
    dtype, f = _acc(p)
    d = np.diag(S)[:p]
    y = _l_mul(S, p, d.astype(dtype)[:, None] * _lt_mul(S, p, z, dtype), dtype)
    az = np.zeros(z.shape, dtype=dtype)
    zz = z.astype(dtype)
    for r0 in range(0, p, _BLOCK):
        r1 = min(p, r0 + _BLOCK)
        az[r0:r1] = A[r0:r1, :p].astype(dtype) @ zz
    bound = f * p * U * _abs_l_mul(S, p, np.abs(d)[:, None] * _abs_lt_mul(S, p, np.abs(z)))
    ratio = _worst_ratio(az - y, bound)
    assert ratio <= 1.0, f"factor probe residual is {ratio:.3g} x its bound (p = {p})"
    return ratio


def check_ep(A, S, v, p, ep):
    """ep == -storage[p-1][p-1] exactly, and v'Av = -ep to (p^2 + 2) u sum |v_i A_ij v_j|."""
    assert ep == -S[p - 1, p - 1] and np.signbit(ep) == np.signbit(-S[p - 1, p - 1]), (ep, S[p - 1, p - 1])
    dtype, f = _acc(p)
    val, mag = _quad(A, v, p, dtype)
    ratio = _worst_ratio(val + dtype(ep), f * (p * p + 2) * U * mag)
    assert ratio <= 1.0, f"v'Av + ep is {ratio:.3g} x its bound (p = {p})"
    return ratio


def check_quad(Fk, v, p, gk, sign):
    """g_k = sign v' F_k v (sign +1 LMIOracle, -1 LMI0Oracle) to (p^2 + 2) u sum |v_i F_ij v_j|."""
    dtype, f = _acc(p)
    val, mag = _quad(Fk, v, p, dtype)
    ratio = _worst_ratio(dtype(gk) - sign * val, f * (p * p + 2) * U * mag)
    assert ratio <= 1.0, f"g_k - sign v'F_k v is {ratio:.3g} x its bound (p = {p})"
    return ratio


def check_exact(storage, pos, ep, expected):
    """`pos`, storage[:rows, :rows] and ep (sign bit included: -0.0 for a zero pivot) against one case of an
    ExactPencil, bit for bit.  `expected` is what ExactPencil.case returned, the matrix included."""
    _, s_exp, pos_exp, ep_exp = expected
    assert tuple(pos) == pos_exp, (pos, pos_exp)
    rows = s_exp.shape[0]
    if not np.array_equal(storage[:rows, :rows], s_exp):  # the quick comparison first: 52M entries at m = 7201
        np.testing.assert_array_equal(storage[:rows, :rows], s_exp)
    if ep_exp is not None:
        assert ep == ep_exp and np.signbit(ep) == np.signbit(ep_exp), (ep, ep_exp)


def expected_sqrt(S):
    """LDLTMgr::sqrt (ldlt_mgr.rs:129-140) from storage: R[i][i] = sqrt(S[i][i]), R[i][j > i] = S[j][i] * R[i][i],
    zeros below.  One correctly rounded sqrt and one product per entry: an implementation must match bit for bit."""
    root = np.sqrt(np.diag(S))
    r = np.triu(S.T * root[:, None], 1)
    r[np.arange(len(root)), np.arange(len(root))] = root
    return r
