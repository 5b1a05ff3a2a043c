"""CPU reference of the batched profit loops (include/ellhip_batch_profit.h): the reference's `ProfitOracle`,
`ProfitRbOracle` and `ProfitOracleQ` (src/oracles/profit_oracle.rs) and its drivers `cutting_plane_optim`
(src/cutting_plane.rs:286-313) and `cutting_plane_optim_q` (:331-374), restated in scalar Python floats (IEEE f64, one
rounding per operation, nothing contracted) over the CPU oracle's spaces (oracle.OracleEll / oracle.OracleEllStable).  Test
infrastructure, not product code.

`exp` and `log` are a parameter of every oracle: ELL = (ell_exp, ell_log), the restatement of csrc/ell_math.hpp operation by
operation, or LIBM = (math.exp, math.log).  The device runs ELL, so its loops are compared with the ELL runs in every bit.

The seeded family (B problems per kind, `family`) and its finished runs are computed once and shared as read-only records.

For the edge tests (tests/test_batch_profit_edges_cpu.py, tests/test_gpu_batch_profit_edges.py): a second draw for the discrete
kind's stop rules (`edge_family`), a table of synthetic oracle states for the retry branch (`retry_table`), the exact ties of
round() (`tie_list`), extreme arguments and starts, and answers that do not come from the restatement -- the problem's closed
form and objective under mpmath (`closed_form`, `profit_at`) and the best integer point by brute force (`discrete_best`).
Divisions go through `fdiv`, which returns what IEEE division returns where a Python float raises."""
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


def fdiv(a, b):
    """a / b as IEEE f64 divides: one rounding, and +-inf or NaN where Python raises ZeroDivisionError"""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


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
                return [fdiv(self.q[0], den) - a[0], fdiv(self.q[1], den) - a[1]], fj
        return None

    def assess_optim(self, y, gamma):
        """((grad, beta), shrunk, gamma)"""
        cut = self.assess_feas(y, gamma)
        if cut is not None:
            return cut, False, gamma
        a = self.elasticities
        exp_val = self.exp(self.log_cobb)
        gamma = exp_val - self.vx
        return ([fdiv(self.q[0], exp_val) - a[0], fdiv(self.q[1], exp_val) - a[1]], 0.0), True, gamma


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


def run_optim_q(omega, space, gamma, max_iters=MAX_ITERS, tol=TOL, trace=None):
    """cutting_plane_optim_q (:331-374).  trace: a list that receives (retry, shrunk, CutStatus) of every round."""
    x_best, status, niter, retry, retries = None, SUCCESS, max_iters, False, 0
    for it in range(max_iters):
        x = [float(v) for v in space.xc]
        (g, beta), shrunk, x_q, more_alt, gamma = omega.assess_optim_q(x, gamma, retry)
        retries += retry
        if shrunk:
            x_best = np.array(x_q)
            retry = False
        st = space.update_q(g, beta)
        if trace is not None:
            trace.append((not more_alt, bool(shrunk), st))
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


# ---- the edge family: the discrete kind's stop rules ----------------------------------------------------------------------------
EDGE_B = 1500
EDGE_SEED = 14
EDGE_TOLS = (1e-6, 1e-3)


@functools.lru_cache(maxsize=None)
def edge_family(B=EDGE_B, seed=EDGE_SEED):
    """`family`'s draw with the limit k from uniform(0.5, 60): small limits put integer points on and beside the bound"""
    rng = np.random.default_rng(seed)
    params = np.stack([rng.uniform(10.0, 30.0, B), rng.uniform(20.0, 60.0, B), rng.uniform(0.5, 60.0, B)], axis=1)
    a = np.stack([rng.uniform(0.05, 0.3, B), rng.uniform(0.2, 0.5, B)], axis=1)
    v = np.stack([rng.uniform(5.0, 20.0, B), rng.uniform(20.0, 50.0, B)], axis=1)
    vparams = np.stack([rng.uniform(0.001, 0.005, B), rng.uniform(0.003, 0.01, B), rng.uniform(0.5, 1.5, B),
                        rng.uniform(0.5, 1.5, B), rng.uniform(0.5, 1.5, B)], axis=1)
    xc0 = rng.uniform(-1.0, 3.0, (B, 2))
    for arr in (params, a, v, vparams, xc0):
        arr.setflags(write=False)
    return params, a, v, vparams, xc0


# Found by a CPU search over the 1500 members at tol = 1e-6 (the search is `edge_paths` over range(EDGE_B));
# tests/test_batch_profit_edges_cpu.py derives the paths of the selected members again.  Keyed by `stable`.
EDGE_TOL_ON_NOEFFECT = {False: (369, 390, 672, 777, 976, 1017), True: (606, 919, 1273)}      # path (b)
EDGE_NOEFFECT_MIDRUN = {False: ((124, 26), (286, 23), (444, 23)),                               # path (c): (member, round j)
                        True: ((82, 18), (103, 25), (445, 27), (525, 22), (689, 23), (1100, 30))}
EDGE_MEMBERS = tuple(sorted(set(range(100)) | {b for s in (False, True) for b in EDGE_TOL_ON_NOEFFECT[s]}
                            | {b for s in (False, True) for b, _ in EDGE_NOEFFECT_MIDRUN[s]}))


def edge_oracle(b, fns=ELL):
    params, a, v, _, _ = edge_family()
    return make_oracle(DISCRETE, tuple(params[b]), a[b], v[b], None, fns)


def edge_space(b, stable):
    return fresh(edge_family()[4][b], stable)


@functools.lru_cache(maxsize=None)
def edge_solve(b, stable, tol, max_iters=MAX_ITERS):
    """member b of the edge family from its fresh space, gamma = 0; `trace` is run_optim_q's, one entry per round"""
    omega, trace = edge_oracle(b), []
    rec = run_optim_q(omega, edge_space(b, stable), 0.0, max_iters, tol, trace)
    rec["idx"], rec["yd"] = oracle_state(omega)
    rec["trace"] = tuple(trace)
    return _freeze(rec)


def edge_paths(rec):
    """which of the stop rules' paths a finished discrete run took: "a" it ended at the tolerance on a Success round, "b" it
    ended by the tolerance test on a NoEffect round, ("c", j) round j was NoEffect and not the run's last"""
    out, trace = set(), rec["trace"]
    at_tol = rec["status"] == SUCCESS and rec["niter"] == len(trace) - 1
    if at_tol and trace[-1][2] == SUCCESS:
        out.add("a")
    if at_tol and trace[-1][2] == NOEFFECT:
        out.add("b")
    out |= {("c", j) for j, t in enumerate(trace[:-1]) if t[2] == NOEFFECT}
    return out


# ---- independent answers: the closed form, the objective, the best integer point ---------------------------------------------
MP_PREC = 160   # bits


def _mp():
    import mpmath
    return mpmath


def closed_form(params, a, v):
    """(gamma*, (x1*, x2*)) of max pA x1^a0 x2^a1 - v0 x1 - v1 x2 subject to x1 <= k, under mpmath.  The stationary point
    has a_i R = v_i x_i with R the revenue, so R^(1 - a0 - a1) = pA (a0/v0)^a0 (a1/v1)^a1 and gamma* = R (1 - a0 - a1); if its
    x1 exceeds k the bound is active and x2 maximises the concave pA k^a0 x2^a1 - v1 x2."""
    mp = _mp()
    with mp.workprec(MP_PREC):
        f = mp.mpf
        pA, k = f(float(params[0])) * f(float(params[1])), f(float(params[2]))
        a0, a1, v0, v1 = f(float(a[0])), f(float(a[1])), f(float(v[0])), f(float(v[1]))
        F = (pA * (a0 / v0) ** a0 * (a1 / v1) ** a1) ** (1 / (1 - a0 - a1))
        x1 = a0 * F / v0
        if x1 <= k:
            return F * (1 - a0 - a1), (x1, a1 * F / v1)
        x2 = (a1 * pA * k ** a0 / v1) ** (1 / (1 - a1))
        return pA * k ** a0 * x2 ** a1 - v0 * k - v1 * x2, (k, x2)


def profit_terms(y, params, a, v):
    """(revenue, cost) at the loop's point y = (ln x1, ln x2), under mpmath"""
    mp = _mp()
    with mp.workprec(MP_PREC):
        f = mp.mpf
        y0, y1 = f(float(y[0])), f(float(y[1]))
        revenue = f(float(params[0])) * f(float(params[1])) * mp.exp(f(float(a[0])) * y0 + f(float(a[1])) * y1)
        return revenue, f(float(v[0])) * mp.exp(y0) + f(float(v[1])) * mp.exp(y1)


def profit_at(y, params, a, v):
    """the objective at the loop's point y = (ln x1, ln x2), under mpmath"""
    mp = _mp()
    with mp.workprec(MP_PREC):
        revenue, cost = profit_terms(y, params, a, v)
        return revenue - cost


def discrete_best(params, a, v):
    """(gamma, (x1, x2)): the maximum over the integer points x1 in [1, floor(k)], x2 in [1, 4 ceil(x2*)] by brute force in
    float64 (x2* is the continuous optimum's, and the best x2 of a fixed x1 <= x1* is below it); None if k < 1"""
    _, (_, x2s) = closed_form(params, a, v)
    n1, n2 = int(math.floor(float(params[2]))), 4 * int(math.ceil(float(x2s)))
    if n1 < 1:
        return None
    x1 = np.arange(1, n1 + 1, dtype=np.float64)[:, None]
    x2 = np.arange(1, n2 + 1, dtype=np.float64)[None, :]
    val = float(params[0]) * float(params[1]) * x1 ** float(a[0]) * x2 ** float(a[1]) - float(v[0]) * x1 - float(v[1]) * x2
    i, j = np.unravel_index(np.argmax(val), val.shape)
    return float(val[i, j]), (float(x1[i, 0]), float(x2[0, j]))


@functools.lru_cache(maxsize=None)
def solve_libm(b):
    """the plain member b of the family on Ell with libm's exp and log"""
    return _freeze(run(PLAIN, family_oracle(PLAIN, b, LIBM), fresh(family()[4][b]), 0.0))


def eps_units(gamma, y, params, a, v):
    """|gamma - profit_at(y)| in units of eps (revenue + cost): gamma is exp_val - vx, two terms that each carry a few eps"""
    mp = _mp()
    with mp.workprec(MP_PREC):
        revenue, cost = profit_terms(y, params, a, v)
        return float(abs(mp.mpf(float(gamma)) - (revenue - cost)) / (mp.mpf(2) ** -52 * (revenue + cost)))


def libm_figures():
    """(worst |gamma - gamma*| / gamma*, worst eps_units) over the family's plain runs with libm and the libm pin"""
    params, a, v, _, _ = family()
    cases = [(solve_libm(b), params[b], a[b], v[b]) for b in range(FAMILY_B)] + [(pin_run(PLAIN, LIBM), PIN_PARAMS, PIN_A, PIN_V)]
    gap = units = 0.0
    for rec, p, aa, vv in cases:
        star = closed_form(p, aa, vv)[0]
        gap = max(gap, float(abs(_mp().mpf(rec["gamma"]) - star) / star))
        units = max(units, eps_units(rec["gamma"], rec["x_best"], p, aa, vv))
    return gap, units


# What libm_figures() gave, rounded up in the third digit (tests/test_batch_profit_edges_cpu.py measures them again): the
# device tests' bounds are multiples of these two, not of anything an ell_exp / ell_log or device run gave.
LIBM_GAP = 7.39e-11     # measured 7.3808e-11
LIBM_UNITS = 4.81       # measured 4.8079


# ---- the synthetic table for the retry branch of assess_optim_q ----------------------------------------------------------------
RETRY_B = 192
RETRY_SEED = 5


def wide_step(oracles, x, gamma, retry=None):
    """one assess_optim_q (retry is None: assess_optim) per oracle: the arguments, the oracles' state before the call
    (idx, yd) and what the wide call must return"""
    before = [oracle_state(om) for om in oracles]
    x, gamma = np.asarray(x, dtype=np.float64), np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (len(oracles),)))
    if retry is None:
        outs = [om.assess_optim([float(x[b, 0]), float(x[b, 1])], float(gamma[b])) for b, om in enumerate(oracles)]
        outs = [(o[0], o[1], x[b], True, o[2]) for b, o in enumerate(outs)]
    else:
        retry = np.array(np.broadcast_to(np.asarray(retry, dtype=np.int32), (len(oracles),)))
        outs = [om.assess_optim_q([float(x[b, 0]), float(x[b, 1])], float(gamma[b]), bool(retry[b]))
                for b, om in enumerate(oracles)]
    want = dict(grad=np.array([o[0][0] for o in outs]), beta=np.array([o[0][1] for o in outs]),
                shrunk=np.array([o[1] for o in outs]), x_q=np.array([o[2] for o in outs]),
                more=np.array([o[3] for o in outs]), gamma=np.array([o[4] for o in outs]))
    step = dict(x=x, gamma=gamma, retry=retry, want=want, idx=np.array([s[0] for s in before]),
                yd=np.array([s[1] for s in before]))
    for arr in list(step.values()) + list(want.values()):
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return step


@functools.lru_cache(maxsize=None)
def retry_table(B=RETRY_B, seed=RETRY_SEED):
    """B discrete problems and five wide calls, with what each must return (the CPU oracles', ell_exp / ell_log):
      0  a call that leaves the cursor at 0 (even members: a cut from the limit) or at 1 (odd: a cut from constraint 1);
      1  a feasible call at x0 that makes yd; a third of the members have k = m + 0.7 and x0[0] = ln(m + 0.6), so that
         yd[0] = ln(m + 1) > ln k;
      2  retry = 1 at x1 != x0 with gamma well below, at or well above what call 1 left;
      3  retry = 1 again at another point, which shows the cursor and yd that call 2 stored;
      4  retry = 0 at x0, which shows what call 3 stored.
    Returns (params, a, v, steps)."""
    rng = np.random.default_rng(seed)
    params, a, v, _, _ = (np.array(t) for t in family(B, seed))
    near = np.arange(B) % 3 == 2
    params[near, 2] = np.floor(params[near, 2]) + 0.7
    oracles = [make_oracle(DISCRETE, tuple(params[b]), a[b], v[b]) for b in range(B)]
    logk = np.log(params[:, 2])
    even = np.arange(B) % 2 == 0
    steps = [wide_step(oracles, np.stack([np.where(even, logk + 1.0, logk - 1.0), np.zeros(B)], axis=1),
                       np.where(even, 0.0, 1e9), 0)]
    x0 = np.stack([np.where(near, np.log(np.floor(params[:, 2]) + 0.6), logk - rng.uniform(0.3, 1.5, B)),
                   rng.uniform(-1.0, 4.0, B)], axis=1)
    revenue = np.exp(np.log(params[:, 0] * params[:, 1]) + a[:, 0] * x0[:, 0] + a[:, 1] * x0[:, 1])
    cost = v[:, 0] * np.exp(x0[:, 0]) + v[:, 1] * np.exp(x0[:, 1])
    gamma0 = (revenue - cost) - rng.choice([0.5, 1e-2, 1e-4], B) * revenue   # feasible at x0, and gamma0 + vx > 0
    steps.append(wide_step(oracles, x0, gamma0, 0))
    g1 = steps[-1]["want"]["gamma"]
    mode = rng.integers(0, 3, B)
    gamma1 = np.where(mode == 0, g1 - 0.5 * np.abs(g1) - 50.0, np.where(mode == 1, g1 + 0.5 * np.abs(g1) + 50.0, g1))
    steps.append(wide_step(oracles, x0 + rng.uniform(-0.5, 0.5, (B, 2)), gamma1, 1))
    steps.append(wide_step(oracles, x0 + rng.uniform(-0.5, 0.5, (B, 2)), steps[-1]["want"]["gamma"], 1))
    steps.append(wide_step(oracles, x0, steps[-1]["want"]["gamma"], 0))
    for arr in (params, a, v):
        arr.setflags(write=False)
    return params, a, v, tuple(steps)


def retry_kinds(step):
    """what each member's retry call was -- "cut0" / "cut1": a feasibility cut at yd from constraint 0 / 1, "shrunk" -- and
    the sign of beta's shift term g.(yd - y)"""
    w, y = step["want"], step["x"]
    kinds, signs = [], []
    for b in range(len(w["beta"])):
        g, yd = w["grad"][b], w["x_q"][b]
        kinds.append("shrunk" if w["shrunk"][b] else "cut0" if (g[0], g[1]) == (1.0, 0.0) else "cut1")
        signs.append(float(np.sign((0.0 + g[0] * (yd[0] - y[b, 0])) + g[1] * (yd[1] - y[b, 1]))))
    return kinds, signs


# ---- ties of round(), the zero clamp, extreme and non-finite arguments -------------------------------------------------------
def ulp_neighbours(y):
    return [float(np.nextafter(y, -INF)), y, float(np.nextafter(y, INF))]


@functools.lru_cache(maxsize=None)
def tie_list():
    """(k, y) with ell_exp(y) == k + 0.5 exactly, y among ell_log(k + 0.5) and its two neighbours, k = 0 .. 39"""
    return tuple((k, y) for k in range(40) for y in ulp_neighbours(ell_log(k + 0.5)) if ell_exp(y) == k + 0.5)


# a problem that is feasible with gamma = 0 wherever x1, x2 lie in [0.4, 45]: pA = 1800, k = 59.5
TIE_PARAMS, TIE_A, TIE_V = (30.0, 60.0, 59.5), (0.3, 0.5), (5.0, 20.0)


@functools.lru_cache(maxsize=None)
def tie_points():
    """[N][2]: every tie value, ell_log(0.5) (below it exp rounds to 0 and is clamped to 1: yd = +0.0) and their 1-ulp
    neighbours in the first coordinate against a few of them in the second, and the other way round"""
    ys = sorted({t for _, y in tie_list() for t in ulp_neighbours(y)} | set(ulp_neighbours(ell_log(0.5))))
    few = ulp_neighbours(ell_log(0.5)) + ulp_neighbours(tie_list()[len(tie_list()) // 2][1]) + [1.0]
    pts = [(y, o) for y in ys for o in few[::2]] + [(o, y) for y in ys for o in few[1::2]]
    out = np.array(pts)
    out.setflags(write=False)
    return out


EXTREME_Y = (709.78, 710.0, 745.0, -745.2, -746.0, INF, -INF, math.nan)


def extreme_calls():
    """(x [N][2], gamma [N]) for wide calls on TIE_PARAMS: every pair of an extreme y with an ordinary coordinate on either
    side and with itself at gamma = 0, then x = (1, 1) at gamma = -vx exactly, below -vx, +inf, 1e308 and NaN"""
    xs = [(y, 1.0) for y in EXTREME_Y] + [(1.0, y) for y in EXTREME_Y] + [(y, y) for y in EXTREME_Y]
    gam = [0.0] * len(xs)
    vx = TIE_V[0] * ell_exp(1.0) + TIE_V[1] * ell_exp(1.0)
    for g in (-vx, -vx - 1.0, -1e9, INF, 1e308, math.nan):
        xs.append((1.0, 1.0))
        gam.append(g)
    return np.array(xs), np.array(gam)


# loops that start outside the finite range: (xc0, kappa, gamma0)
EXTREME_STARTS = {"xc": ((-800.0, 720.0), KAPPA, 0.0), "kappa": ((1.0, 1.0), 1e300, 0.0),
                  "gamma_high": ((1.0, 1.0), KAPPA, 1e300), "gamma_low": ((1.0, 1.0), KAPPA, -1e9)}
EXTREME_ITERS = 50
