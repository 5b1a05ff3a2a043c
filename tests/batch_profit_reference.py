"""CPU reference of the batched profit loops (include/ellhip_batch_profit.h): the reference's `ProfitOracle`,
`ProfitRbOracle` and `ProfitOracleQ` (src/oracles/profit_oracle.rs) and its drivers `cutting_plane_optim`
(src/cutting_plane.rs:286-313) and `cutting_plane_optim_q` (:331-374), restated in scalar Python floats (IEEE f64, one
rounding per operation, nothing contracted) over the CPU oracle's spaces (oracle.OracleEll / oracle.OracleEllStable).  Test
infrastructure, not product code.

`exp` and `log` are a parameter of every oracle: ELL = (ell_exp, ell_log), the restatement of csrc/ell_math.hpp operation by
operation, or LIBM = (math.exp, math.log).  The device runs ELL, so its loops are compared with the ELL runs in every bit.

The seeded family (B problems per kind, `family`) and its finished runs are computed once and shared as read-only records."""
import functools
import math
import struct

import numpy as np

from oracle import oracle as O

SUCCESS, NOSOLN, NOEFFECT, UNKNOWN = 0, 1, 2, 3
PLAIN, ROBUST, DISCRETE = 0, 1, 2
KINDS = {"plain": PLAIN, "robust": ROBUST, "discrete": DISCRETE}
KAPPA = 100.0
TOL = 1e-20          # Options::default()
MAX_ITERS = 2000
INF = math.inf


# ---- csrc/ell_math.hpp, operation by operation --------------------------------------------------------------------------------
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u & 0xFFFFFFFFFFFFFFFF))[0]


LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
INV_LN2 = 1.44269504088896338700e+00
assert bits(LN2_HI) == 0x3FE62E42FEE00000 and bits(LN2_LO) == 0x3DEA39EF35793C76 and bits(INV_LN2) == 0x3FF71547652B82FE
EXP_COEF = [1.0 / 1307674368000.0, 1.0 / 87178291200.0, 1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0,
            1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5]
LOG_COEF = [2.0 / 25.0, 2.0 / 23.0, 2.0 / 21.0, 2.0 / 19.0, 2.0 / 17.0, 2.0 / 15.0, 2.0 / 13.0, 2.0 / 11.0, 2.0 / 9.0,
            2.0 / 7.0, 2.0 / 5.0, 2.0 / 3.0]
TWO_M1000 = from_bits(0x0170000000000000)


def ell_exp(x):
    if x != x:
        return x + x
    if x > 710.0:
        return INF
    if x < -746.0:
        return 0.0
    kf = x * INV_LN2
    k = int(kf - 0.5 if x < 0.0 else kf + 0.5)   # truncation, as (int)
    kd = float(k)
    hi = x - kd * LN2_HI
    lo = kd * LN2_LO
    r = hi - lo
    e = (hi - r) - lo
    p = EXP_COEF[0]
    for c in EXP_COEF[1:]:
        p = p * r + c
    q = (r * r) * p
    t = 1.0 + r
    terr = (1.0 - t) + r
    y = t + (terr + (q + e))
    if k > 1023:
        return from_bits(bits(y) + ((k - 1) << 52)) * 2.0
    if k < -1021:
        return from_bits(bits(y) + ((k + 1000) << 52)) * TWO_M1000
    return from_bits(bits(y) + (k << 52))


def ell_log(x):
    if x != x:
        return x + x
    u = bits(x)
    if (u << 1) & 0xFFFFFFFFFFFFFFFF == 0:
        return -INF
    if u >> 63:
        return math.nan
    if u == 0x7FF0000000000000:
        return x
    k = 0
    if u >> 52 == 0:
        u = bits(x * 18014398509481984.0)
        k = -54
    k += (u >> 52) - 1023
    mant = u & 0x000FFFFFFFFFFFFF
    if mant >= 0x0006A09E667F3BCD:
        mant |= 0x3FE0000000000000
        k += 1
    else:
        mant |= 0x3FF0000000000000
    f = from_bits(mant) - 1.0
    dk = float(k)
    s = f / (2.0 + f)
    z = s * s
    R = LOG_COEF[0]
    for c in LOG_COEF[1:]:
        R = R * z + c
    R = R * z
    hfsq = (0.5 * f) * f
    if k == 0:
        return f - (hfsq - s * (hfsq + R))
    return dk * LN2_HI - ((hfsq - (s * (hfsq + R) + dk * LN2_LO)) - f)


def libm_exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def libm_log(x):
    if x != x:
        return x
    if x == 0.0:
        return -INF
    if x < 0.0:
        return math.nan
    return math.log(x)


ELL = (ell_exp, ell_log)
LIBM = (libm_exp, libm_log)


EXP_SPECIALS = [0.0, -0.0, INF, -INF, math.nan, 709.782712893384, 709.7827128933841, 709.9, 710.0, 710.5, 1e308, -708.3964185322641,
                -708.5, -744.0, -745.1332191019411, -745.1332191019412, -745.5, -746.0, -746.5, -1e308, 5e-324, -5e-324,
                1e-300, 1.0, -1.0, 0.34657359027997264, -0.34657359027997264, 0.5 * 0.6931471805599453, 1e-17, -1e-17]
LOG_SPECIALS = [0.0, -0.0, INF, -INF, math.nan, -1.0, -5e-324, 5e-324, 2.2250738585072014e-308, 2.225073858507201e-308,
                1e-310, 1.7976931348623157e308, 1.0, 1.0000000000000002, 0.9999999999999999, 1.4142135623730951,
                1.414213562373095, 0.7071067811865476, 0.7071067811865475, 2.0, 0.5, 3.0, 10.0, 2.718281828459045]


def math_sweep(fn, count=100_000, seed=7):
    """seeded arguments for "exp" / "log" (float64 array of `count`), the special values first"""
    rng = np.random.default_rng(seed)
    if fn == "exp":
        head = np.array(EXP_SPECIALS)
        m = count - head.size
        parts = [rng.uniform(-746.0, 710.0, m // 2), rng.uniform(-1.0, 1.0, m // 4), rng.uniform(-40.0, 40.0, m // 8),
                 rng.normal(size=m // 16) * 1e-5, rng.uniform(-745.2, -707.0, m // 32)]
        rest = m - sum(p.size for p in parts)
        parts.append((rng.integers(-1070, 1020, rest) + 0.5) * 0.6931471805599453 + rng.normal(size=rest) * 1e-9)
    else:
        head = np.array(LOG_SPECIALS)
        m = count - head.size
        parts = [rng.integers(1, 0x7FF0000000000000, m // 2, dtype=np.int64).view(np.float64), rng.uniform(0.5, 2.0, m // 4),
                 1.0 + rng.normal(size=m // 8) * 1e-6, rng.uniform(1.0, 1e6, m // 16)]
        rest = m - sum(p.size for p in parts)
        parts.append(np.rint(rng.uniform(1.0, 3000.0, rest)))   # what round(exp(y)) hands to ln
    out = np.concatenate([head] + parts)
    assert out.size == count
    return out


def host_eval(fn, xs):
    """csrc/ell_math.hpp compiled by plain g++ (tests/cpp/ell_math_host.cpp) over an array"""
    import subprocess
    from cpp_build import build_host_tool
    exe = build_host_tool("ell_math_host.cpp")
    out = subprocess.run([exe, fn], input=np.ascontiguousarray(xs, dtype=np.float64).tobytes(), capture_output=True, check=True,
                         timeout=120).stdout
    return np.frombuffer(out, dtype=np.float64)


def rust_round(v):
    """f64::round: half away from zero (np.round and Python's round are half to even)"""
    if v != v or v in (INF, -INF):
        return v
    a = abs(v)
    r = float(math.floor(a))
    if a - r >= 0.5:
        r += 1.0
    return math.copysign(r, v)


# ---- the oracles ----------------------------------------------------------------------------------------------------------------
class ProfitOracle:
    def __init__(self, params, elasticities, price_out, fns=ELL):
        self.exp, self.log = fns
        unit_price, scale, limit = params
        self.log_p_scale = self.log(unit_price * scale)
        self.log_k = self.log(limit)
        self.idx = -1
        self.price_out = [float(price_out[0]), float(price_out[1])]
        self.elasticities = [float(elasticities[0]), float(elasticities[1])]
        self.log_cobb, self.vx, self.q = 0.0, 0.0, [0.0, 0.0]

    def assess_feas(self, y, gamma):
        a = self.elasticities
        for _ in range(2):
            self.idx += 1
            if self.idx == 2:
                self.idx = 0
            if self.idx == 0:
                fj = y[0] - self.log_k
            else:
                self.log_cobb = self.log_p_scale + ((0.0 + a[0] * y[0]) + a[1] * y[1])
                self.q = [self.price_out[0] * self.exp(y[0]), self.price_out[1] * self.exp(y[1])]
                self.vx = self.q[0] + self.q[1]
                fj = self.log(gamma + self.vx) - self.log_cobb
            if fj > 0.0:
                if self.idx == 0:
                    return [1.0, 0.0], fj
                den = gamma + self.vx
                return [self.q[0] / den - a[0], self.q[1] / den - a[1]], fj
        return None

    def assess_optim(self, y, gamma):
        """((grad, beta), shrunk, gamma)"""
        cut = self.assess_feas(y, gamma)
        if cut is not None:
            return cut, False, gamma
        a = self.elasticities
        exp_val = self.exp(self.log_cobb)
        gamma = exp_val - self.vx
        return ([self.q[0] / exp_val - a[0], self.q[1] / exp_val - a[1]], 0.0), True, gamma


class ProfitRbOracle:
    def __init__(self, params, elasticities, price_out, vparams, fns=ELL):
        e1, e2, e3, e4, e5 = vparams
        self.uie = [e1, e2]
        self.elasticities = [float(elasticities[0]), float(elasticities[1])]
        self.omega = ProfitOracle((params[0] - e3, params[1], params[2] - e4), elasticities,
                                  [price_out[0] + e5, price_out[1] + e5], fns)

    def assess_optim(self, y, gamma):
        a_rb = list(self.elasticities)
        for i in range(2):
            a_rb[i] += -self.uie[i] if y[i] > 0.0 else self.uie[i]
        self.omega.elasticities = a_rb
        return self.omega.assess_optim(y, gamma)


class ProfitOracleQ:
    def __init__(self, params, elasticities, price_out, fns=ELL):
        self.omega = ProfitOracle(params, elasticities, price_out, fns)
        self.yd = [0.0, 0.0]

    def assess_optim_q(self, y, gamma, retry):
        """((grad, beta), shrunk, x_q, more_alt, gamma)"""
        om = self.omega
        if not retry:
            cut = om.assess_feas(y, gamma)
            if cut is not None:
                return cut, False, [y[0], y[1]], True, gamma
            x_disc = [rust_round(om.exp(y[0])), rust_round(om.exp(y[1]))]
            x_disc = [1.0 if v == 0.0 else v for v in x_disc]
            self.yd = [om.log(x_disc[0]), om.log(x_disc[1])]
        (grad, beta), shrunk, gamma = om.assess_optim(self.yd, gamma)
        beta = beta + ((0.0 + grad[0] * (self.yd[0] - y[0])) + grad[1] * (self.yd[1] - y[1]))
        return (grad, beta), shrunk, list(self.yd), not retry, gamma


def make_oracle(kind, params, a, v, vparams=None, fns=ELL):
    if kind == PLAIN:
        return ProfitOracle(params, a, v, fns)
    if kind == ROBUST:
        return ProfitRbOracle(params, a, v, vparams, fns)
    return ProfitOracleQ(params, a, v, fns)


def oracle_state(omega):
    """(idx, yd) as the device handle keeps them"""
    core = omega.omega if hasattr(omega, "omega") else omega
    return core.idx, list(getattr(omega, "yd", [0.0, 0.0]))


# ---- the drivers ----------------------------------------------------------------------------------------------------------------
def space_record(space):
    return dict(mq=np.array(space.mq), xc=np.array(space.xc), kappa=space.kappa, tsq=space.tsq)


def run_optim(omega, space, gamma, max_iters=MAX_ITERS, tol=TOL):
    """cutting_plane_optim (:286-313).  status: the CutStatus that ended the loop, Success for the tolerance or max_iters."""
    x_best, status, niter = None, SUCCESS, max_iters
    for it in range(max_iters):
        x = [float(v) for v in space.xc]
        (g, beta), shrunk, gamma = omega.assess_optim(x, gamma)
        if shrunk:
            x_best = np.array(x)
            st = space.update_central_cut(g, beta)
        else:
            st = space.update_bias_cut(g, beta)
        if st != SUCCESS or space.tsq < tol:
            niter, status = it, st
            break
    return dict(x_best=x_best, niter=niter, gamma=gamma, status=status, retries=0, **space_record(space))


def run_optim_q(omega, space, gamma, max_iters=MAX_ITERS, tol=TOL):
    """cutting_plane_optim_q (:331-374)"""
    x_best, status, niter, retry, retries = None, SUCCESS, max_iters, False, 0
    for it in range(max_iters):
        x = [float(v) for v in space.xc]
        (g, beta), shrunk, x_q, more_alt, gamma = omega.assess_optim_q(x, gamma, retry)
        retries += retry
        if shrunk:
            x_best = np.array(x_q)
            retry = False
        st = space.update_q(g, beta)
        if st == SUCCESS:
            retry = False
        elif st == NOSOLN:
            niter, status = it, st
            break
        elif st == NOEFFECT:
            if not more_alt:
                niter, status = it, st
                break
            retry = True
        if space.tsq < tol:
            niter = it
            break
    return dict(x_best=x_best, niter=niter, gamma=gamma, status=status, retries=retries, **space_record(space))


def run(kind, omega, space, gamma, max_iters=MAX_ITERS, tol=TOL):
    return (run_optim_q if kind == DISCRETE else run_optim)(omega, space, gamma, max_iters, tol)


def fresh(xc0, stable=False, kappa=KAPPA):
    return (O.OracleEllStable if stable else O.OracleEll).new_with_scalar(kappa, np.asarray(xc0, dtype=np.float64))


# ---- the reference's pinned cases (src/oracles/profit_oracle.rs:172-225) --------------------------------------------------------
PIN_PARAMS, PIN_A, PIN_V, PIN_VPARAMS = (20.0, 40.0, 30.5), (0.1, 0.4), (10.0, 35.0), (0.003, 0.007, 1.0, 1.0, 1.0)
PINS = {PLAIN: 83, ROBUST: 90, DISCRETE: 29}


def pin_space():
    return O.OracleEll.new(np.array([100.0, 100.0]), np.array([0.0, 0.0]))


def pin_run(kind, fns=ELL):
    return run(kind, make_oracle(kind, PIN_PARAMS, PIN_A, PIN_V, PIN_VPARAMS, fns), pin_space(), 0.0)


# ---- the seeded family ----------------------------------------------------------------------------------------------------------
FAMILY_B = 200
FAMILY_SEED = 2024


@functools.lru_cache(maxsize=None)
def family(B=FAMILY_B, seed=FAMILY_SEED):
    """params [B][3], a [B][2], v [B][2], vparams [B][5], xc0 [B][2]; the same draw for every kind"""
    rng = np.random.default_rng(seed)
    params = np.stack([rng.uniform(10.0, 30.0, B), rng.uniform(20.0, 60.0, B), rng.uniform(5.0, 60.0, B)], axis=1)
    a = np.stack([rng.uniform(0.05, 0.3, B), rng.uniform(0.2, 0.5, B)], axis=1)
    v = np.stack([rng.uniform(5.0, 20.0, B), rng.uniform(20.0, 50.0, B)], axis=1)
    vparams = np.stack([rng.uniform(0.001, 0.005, B), rng.uniform(0.003, 0.01, B), rng.uniform(0.5, 1.5, B),
                        rng.uniform(0.5, 1.5, B), rng.uniform(0.5, 1.5, B)], axis=1)
    xc0 = rng.uniform(-1.0, 3.0, (B, 2))
    for arr in (params, a, v, vparams, xc0):
        arr.setflags(write=False)
    return params, a, v, vparams, xc0


def family_oracle(kind, b, fns=ELL, B=FAMILY_B):
    params, a, v, vparams, _ = family(B)
    return make_oracle(kind, tuple(params[b]), a[b], v[b], tuple(vparams[b]), fns)


def _freeze(rec):
    for val in rec.values():
        if isinstance(val, np.ndarray):
            val.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def solve(kind, b, stable=False, max_iters=MAX_ITERS, tol=TOL):
    """member b of the family from its fresh space, gamma = 0, with ell_exp / ell_log; the oracle's state afterwards too"""
    omega = family_oracle(kind, b)
    rec = run(kind, omega, fresh(family()[4][b], stable), 0.0, max_iters, tol)
    rec["idx"], rec["yd"] = oracle_state(omega)
    return _freeze(rec)
