"""One EllStable update checked as a map from an observed state to an observed state.

The C ABI shows the packed buffer, xc, kappa and tsq -- not w, z or q.  What can be checked from those alone, element by
element and on each element's own scale, is a set of residual relations: the scratch triangle S the update leaves IS the list
of products the forward solve subtracted, so w can be rebuilt from S exactly; everything behind w follows from it.  No
rescaling identity exists for EllStable (the bug-compatible backward solve reads S, not U), so the relations are bounds.

Every bound is `count * u * (sum of the absolute terms)` with u = 2^-53 and `count` = the largest number of roundings on a
term's path through the kernels plus the checker's own (stated beside each); they hold for any summation order, blocking and
use of fused multiply-adds.  Nothing here is taken from what a GPU returned.  `check_step` returns observed / bound per stage;
a value above 1 (or NaN: a poisoned element read into a result) is a defect.
"""
import itertools
import math
from fractions import Fraction

import numpy as np

U_RND = 2.0 ** -53
C_CALC = 32   # EllCalc: at most 16 roundings on the longest path (parallel_bias_cut_fast -> sigma, rho), each side
TINY = 1e-300


# ------------------------------------------------------------------------------------------------------ inputs
def graded_scales(n, seed, emax):
    """e_i uniform in [-emax, emax] (emax = 0: all zero), the extremes present from n = 2 on."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-emax, emax + 1, n) if emax else np.zeros(n, dtype=np.int64)
    if emax and n >= 2:
        lo, hi = rng.permutation(n)[:2]
        e[lo], e[hi] = -emax, emax
    return e


def graded_factor(n, seed, emax, junk="nan"):
    """util.random_factor graded row by row: U[j][i] = U0[j][i] 2^(e_i - e_j), D_i = d0_i 4^(-e_i), so that with
    g = 2^e * h every w_i, z_i, S[i][j] sits at its own power of two.  junk: what the scratch triangle holds ("nan", "finite":
    noise at each element's own scale, None: zeros).  Returns (buffer, e)."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n)) * (0.1 / np.sqrt(n))
    d0 = 0.5 + rng.random(n)
    e = graded_scales(n, seed + 1, emax)
    a = np.ldexp(1.0, e)
    buf = np.triu(m, 1) * (a[None, :] / a[:, None])
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    if junk == "nan":
        buf[low] = np.nan
    elif junk == "finite":
        buf[low] = (rng.standard_normal((n, n)) * a[:, None])[low]
    buf[np.arange(n), np.arange(n)] = d0 / a ** 2
    return np.ascontiguousarray(buf), e


def graded_grad(rng, e):
    h = rng.standard_normal(len(e))
    h /= np.linalg.norm(h)
    return np.ldexp(h, e)


# ------------------------------------------------------------------------------------------- the checker's own sums
def exact_forward(g, S):
    """w~[i] = g[i] - sum_{j<i} S[i][j], correctly rounded (math.fsum), and sum|terms| per row."""
    n = len(g)
    wt = np.empty(n)
    for i in range(n):
        wt[i] = math.fsum(itertools.chain((g[i],), (-S[i, :i]).tolist()))
    mag = np.abs(g) + np.sum(np.abs(np.tril(S, -1)), axis=1)
    return wt, mag


def exact_prefix(t0, gg):
    """t0 + sum_{k<=j} gg[k] for every j, each correctly rounded (exact rational accumulation)."""
    acc = Fraction(float(t0))
    out = np.empty(len(gg))
    for j, v in enumerate(gg.tolist()):
        acc += Fraction(v)
        out[j] = float(acc)
    return out


def exact_backward_rhs(cz, ST, d):
    """rhs[i] = -cz[i] - sum_{j>i} S[j][i] d[j] (products rounded once, the sum exact) and sum|terms|; ST = S transposed."""
    n = len(cz)
    rhs, mag = np.empty(n), np.empty(n)
    for i in range(n):
        t = ST[i, i + 1:] * d[i + 1:]
        rhs[i] = math.fsum(itertools.chain((-cz[i],), (-t).tolist()))
        mag[i] = abs(cz[i]) + float(np.sum(np.abs(t)))
    return rhs, mag


def _ratio(err, bound, mask=None):
    """max err / bound; 0 where err is exactly 0; NaN if any err is NaN (never silently dropped)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0.0, 0.0, err / np.maximum(bound, TINY))
    if mask is not None:
        r = r[mask]
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------ the check
def check_step(calc, buf0, g, kappa0, cut, xc0, buf1, xc1, kappa1, tsq, status):
    """calc: the project's EllCalc for this n (oracle.Calc); buf0: buffer the update started from (D, U; its scratch
    triangle is never read); cut = (kind, b0, b1 or None); buf1 / xc1 / kappa1 / tsq / status: observed after the update.
    Returns ({stage: observed/bound}, reference status)."""
    kind, b0, b1 = cut
    u = U_RND
    g = np.asarray(g, dtype=np.float64)
    xc0, xc1 = np.asarray(xc0, dtype=np.float64), np.asarray(xc1, dtype=np.float64)
    n = len(g)
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    up = low.T
    U = np.triu(buf0, 1)
    D = np.diag(buf0).copy()
    S = np.where(low, buf1, 0.0)
    out = {}

    # forward solve.  The kernel's w^_i is g_i minus the parked products in some order: at most i additions on a term's path,
    # one more rounding where a fused multiply-add subtracted the unrounded product instead of the parked one: i + 1; the
    # second-order rest (1 + u)^(i+1) - 1 - (i+1)u is covered by counting i + 2.
    wt, mag = exact_forward(g, S)
    B = (np.arange(n) + 2) * u * mag
    relw = B / np.maximum(np.abs(wt), TINY)

    # scratch: S[i][j] = fl(U[j][i] w^_j), w^_j = w~_j + (<= B_j); the checker's own product rounds once more: 2u|P|
    P = U.T * wt[None, :]
    out["scratch"] = _ratio(np.abs(S - P), np.abs(U.T) * (B * (1 + u))[None, :] + 2 * u * np.abs(P), low)

    # tsq.  gg^_i / gg~_i = (1+relw)^2 (1+u)^2 [kernel's z, gg] / (1+u)^4 [w~ rounded, twice; the checker's z, gg]: egg_i.
    # omega: n - 1 additions in any order, 1 for fsum; tsq = kappa omega: one rounding on each side.  (n + 8) u in all.
    z = wt * D
    gg = z * wt
    omega = math.fsum(gg.tolist())
    egg = 2 * relw + relw ** 2 + 6 * u
    eps_om = float(np.sum(egg * np.abs(gg))) / max(abs(omega), TINY) + n * u
    eps_t = eps_om + 2 * u
    tsq_ref = kappa0 * omega
    out["tsq"] = _ratio(abs(tsq - tsq_ref), eps_t * abs(tsq_ref))

    st_ref, (rho, sigma, delta) = calc.dispatch(kind, b0, b1, tsq_ref)
    out["status"] = 0.0 if int(status) == int(st_ref) else np.inf
    if st_ref != 0:   # failed cut: only the scratch triangle may have changed
        same = (np.array_equal(buf1[up | np.eye(n, dtype=bool)], buf0[up | np.eye(n, dtype=bool)])
                and np.array_equal(xc1, xc0) and kappa1 == kappa0)
        out["intact"] = 0.0 if same else np.inf
        return out, st_ref

    # scalars: the kernel evaluated EllCalc at its own tsq^, within eps_t of tsq~.  The sensitivity is EllCalc's own, taken
    # at both ends of that interval; C_CALC u for the roundings inside it (no cancellation worse than 2x on these cuts).
    def sens(x0, xs):
        return max(abs(x - x0) for x in xs) / max(abs(x0), TINY) + C_CALC * u
    ends = [calc.dispatch(kind, b0, b1, tsq_ref * (1 + s * eps_t)) for s in (1.0, -1.0)]
    if any(st != 0 for st, _ in ends):
        e_rho = e_sig = e_del = np.inf   # a branch of EllCalc inside the interval: nothing can be said
    else:
        e_rho = sens(rho, [c[0] for _, c in ends])
        e_sig = sens(sigma, [c[1] for _, c in ends])
        e_del = sens(delta, [c[2] for _, c in ends])
    c_ro = rho / omega                                   # :101, one division each side
    e_c = e_rho + eps_om + 2 * u
    mu = sigma / (1.0 - sigma)                           # :107, d ln mu = e_sig / (1 - sigma); 1 - sigma and the division round
    e_mu = e_sig / abs(1.0 - sigma) + 4 * u
    t0 = omega / mu                                      # :108
    e_t0 = eps_om + e_mu + 2 * u

    out["kappa"] = _ratio(abs(kappa1 - kappa0 * delta), abs(kappa0 * delta) * (e_del + 2 * u))

    # backward solve, on d = xc' - xc0 = -fl(c^ q^).  A term's path: n - i - 1 additions, the product S q, the scaling by c^,
    # the rounding of d_j itself: n - i + 2; the checker's products and fsum: 2 more.  The leading term carries the errors of
    # c^ and z^_i (relw_i, 1 rounding, 2 of the checker's).  A non-zero xc0 hides d_j behind the rounding of xc'_j.
    d = xc1 - xc0
    cz = c_ro * z
    ST = np.ascontiguousarray(S.T)
    rhs, bmag = exact_backward_rhs(cz, ST, d)
    bb = (n - np.arange(n) + 4) * u * bmag + np.abs(cz) * (relw + e_c + 3 * u)
    if np.any(xc0 != 0.0):
        hid = np.abs(xc1) + np.abs(d)
        bb = bb + 2 * u * (hid + np.abs(ST) @ hid)
    out["xc"] = _ratio(np.abs(d - rhs), bb)

    # temp_j = t0 + sum_{k<=j} gg_k, positive for sigma > 0.  The kernels build it from a scan of chunk totals (m = ceil(n/1024) elements per
    # chunk: m - 1 additions, 6 scan steps, up to 16 wave offsets, the exclusive prefix as a difference of two partial sums
    # that are both <= temp_j when m = 1, t0 added, m left-to-right additions): 28 + 2m roundings relative to temp_j, plus
    # what t0 and the gg carry.  For m > 1 the difference can reach past j: an absolute (2m + 6) u omega.
    m = (n + 1023) // 1024
    # (A cut with beta < -tau/n has sigma < 0 and t0 < 0 < gg: |t0| + sum gg stands for temp_j in the rounding terms.)
    pre = exact_prefix(t0, gg)
    E = ((28 + 2 * m) * u * (abs(t0) + np.cumsum(np.abs(gg))) + e_t0 * abs(t0) + np.cumsum(egg * np.abs(gg))
         + ((2 * m + 6) * u * abs(omega) if m > 1 else 0.0))
    relT = E / np.maximum(np.abs(pre), TINY)
    prev = np.concatenate(([t0], pre[:-1]))
    relT_prev = np.concatenate(([e_t0], relT[:-1]))

    # D'_j = D_j (temp_{j-1} / temp_j): a division and a product each side
    Dref = D * (prev / pre)
    out["D"] = _ratio(np.abs(np.diag(buf1) - Dref), np.abs(Dref) * (relT_prev + relT + 6 * u))

    # beta2_j = z_j / temp_j: z^ (relw, 1 rounding; 2 of the checker's), the division each side
    b2 = z / pre
    e_b2 = relw + relT + 6 * u
    # U'[j][l] = U[j][l] + beta2_j S[l][j]: eager forms 2 roundings; the mirrored layout fl(U fl(1 + fl(beta2 w))) with
    # S = fl(U w): 4; the checker's product and sum 2.  beta2_j w_j = gg_j / temp_j >= 0: nothing cancels.
    T = b2[:, None] * ST
    Uref = U + T
    out["U"] = _ratio(np.abs(np.where(up, buf1, 0.0) - Uref), 4 * u * np.abs(U) + np.abs(T) * (e_b2[:, None] + 8 * u), up)
    return out, st_ref


STAGES = ("scratch", "tsq", "status", "intact", "kappa", "xc", "D", "U")


def failures(ratios):
    """Stages whose observed / bound is above 1 or NaN."""
    return sorted(k for k, v in ratios.items() if not (v <= 1.0))


def merge_max(acc, ratios):
    for k, v in ratios.items():
        acc[k] = v if k not in acc or not (v <= acc[k]) else acc[k]
    return acc


# ------------------------------------------------------------- plain-double restatements (reference order, no GPU)
def plain_step(calc, buf, g, kappa, cut, xc, defect=None, prev_scratch=None, small=None):
    """EllStable::update_core in plain sequential double arithmetic (oracle/ell_oracle.c: orc_ellstable_update), with one
    planted defect.  small: index of a small-scale row (for the defects that hide there).  Returns the observables."""
    kind, b0, b1 = cut
    n = len(g)
    mq, xc, w = buf.copy(), np.array(xc, dtype=np.float64), np.array(g, dtype=np.float64)
    lo = 64 if n > 64 else n // 2
    for i in range(1, n):
        wj = w[:i].copy()
        if defect == "stale_w_tile" and i >= lo:          # rows behind the first tile read w of that tile 2e-11 out of date
            wj[:lo] *= 1.0 + 2e-11
        val = mq[:i, i] * wj
        keep = mq[i, 1] if (defect == "scratch_junk" and i == small) else None
        mq[i, :i] = val
        acc = w[i]
        for jj, v in enumerate(val.tolist()):
            if defect == "fwd_term_dropped" and i == small and jj == 1:
                continue
            acc -= v
        w[i] = acc
        if keep is not None:
            mq[i, 1] = keep
    d = np.diag(mq).copy()
    z = w * d
    gg = z * w
    omega = 0.0
    for v in gg.tolist():
        omega += v
    tsq = kappa * omega
    st, (rho, sigma, delta) = calc.dispatch(kind, b0, b1, tsq)
    if st != 0:
        return mq, xc, kappa, tsq, st
    q = z.copy()
    for i in range(n - 1, 0, -1):
        t = mq[i:, i - 1] * q[i:]
        acc = q[i - 1]
        for jj, v in enumerate(t.tolist()):
            if defect == "bwd_term_dropped" and i - 1 == small and jj == n - 1 - i:
                continue
            acc -= v
        q[i - 1] = acc
    xc = xc - (rho / omega) * q
    mu = sigma / (1.0 - sigma)
    oldt = omega / mu
    scr = prev_scratch if defect == "scratch_of_previous_cut" else mq
    for j in range(n - 1):
        temp = oldt + gg[j]
        b2 = z[j] / (oldt if (defect == "beta2_prev_temp" and j == n // 3) else temp)
        if defect == "D_off_by_one":
            mq[j, j] *= temp / (temp + gg[j + 1])
        else:
            mq[j, j] *= oldt / temp
        mq[j, j + 1:] += b2 * scr[j + 1:, j]
        oldt = temp
    mq[n - 1, n - 1] *= oldt / (oldt + gg[n - 1])
    return mq, xc, kappa * delta, tsq, 0


DEFECTS = ("stale_w_tile", "fwd_term_dropped", "bwd_term_dropped", "beta2_prev_temp", "D_off_by_one", "scratch_junk",
           "scratch_of_previous_cut")


def mirrored_run(calc, buf, kappa, cuts):
    """The mirrored layout's arithmetic restated (ellstable_kernels.hpp, StPend): U_base never changes, every use reads
    fl(U_base[j][l] r[j]), a successful cut does r[j] <- r[j] (1 + beta2_j w_j); the buffer is fl(U_base r) at the end.
    Reference summation order.  cuts: [(kind, g, b0, b1)].  Returns (D, U) after the run."""
    n = buf.shape[0]
    base, d, r = np.triu(buf, 1), np.diag(buf).copy(), np.ones(n)
    for kind, g, b0, b1 in cuts:
        ue = base * r[:, None]
        w = np.array(g, dtype=np.float64)
        for i in range(1, n):
            acc = w[i]
            for v in (ue[:i, i] * w[:i]).tolist():
                acc -= v
            w[i] = acc
        z = w * d
        gg = z * w
        omega = 0.0
        for v in gg.tolist():
            omega += v
        st, (rho, sigma, delta) = calc.dispatch(kind, b0, b1, kappa * omega)
        if st != 0:
            continue
        oldt = omega / (sigma / (1.0 - sigma))
        for j in range(n):
            temp = oldt + gg[j]
            d[j] *= oldt / temp
            if j < n - 1:
                r[j] = r[j] * (1.0 + (z[j] / temp) * w[j])
            oldt = temp
        kappa *= delta
    return d, base * r[:, None]


def rel_elementwise(a, b, mask=None):
    """max |a - b| / |b| over the mask, every element on its own scale (0/0 = 0; NaN is kept)."""
    return _ratio(np.abs(np.asarray(a) - np.asarray(b)), np.abs(b), mask)


# ------------------------------------------------------------------- what the CPU file and the GPU files share
SIZES = [2, 3, 63, 64, 65, 127, 128, 129, 257, 300, 1000]   # 64-wide halves, 128-blocks, ragged tails, 1 to 8 chain blocks
CASES = [(n, em) for n in SIZES for em in (0, 10)] + [(129, 20)]
KEEP_XC_AT = 5           # the one cut of eight that starts from the centre the cut before left (non-zero xc0)
MULTI_SIZES = (129, 300)
PERIOD_SIZES = (64, 130, 257)


def case_seed(n, emax):
    return 3000 + 7 * n + emax


_multi_cache = {}


def multi_cut_reference(orc, calc, n, k=6, emax=10):
    """Six successful cuts on the graded factor: the oracle's final (D, U), and how far the plain restatement of the
    mirrored arithmetic is from it, element by element and relatively.  Returns (dev_D, dev_U, (buf, kappa, cuts, D, U))."""
    if n not in _multi_cache:
        from util import mixed_cut, stable_tau
        buf, e = graded_factor(n, case_seed(n, emax) + 1, emax, junk="finite")
        o = orc.OracleEllStable.new_with_matrix(1.5, buf, np.zeros(n))
        rng = np.random.default_rng(n)
        cuts = []
        for i in range(k):
            g = graded_grad(rng, e)
            kind, b0, b1 = mixed_cut(i, g, stable_tau(o, g), rng)
            assert o.update(kind, g, b0, b1) == 0
            cuts.append((kind, g, b0, b1))
        d_o, u_o = np.diag(o.mq).copy(), np.triu(o.mq, 1)
        d_m, u_m = mirrored_run(calc, buf, 1.5, cuts)
        up = np.triu(np.ones((n, n), dtype=bool), 1)
        _multi_cache[n] = (rel_elementwise(d_m, d_o), rel_elementwise(u_m, u_o, up), (buf, 1.5, cuts, d_o, u_o))
    return _multi_cache[n]


class PeriodSeq:
    """A 600-cut adaptive sequence from util.random_factor on the oracle: the cuts, the oracle's status and tsq per cut, and
    its state (mq, xc, kappa) after the numbers of cuts in SNAPS."""
    SNAPS = (250, 251, 255, 256, 257, 300, 512, 600)


_period_cache = {}


def period_sequence(orc, n, with_nosoln, k=600):
    """with_nosoln: util.mixed_cut as it is (every 8th cut fails; cut 255, the 256th update, is one of them); otherwise its
    seven successful entry points in turn (what a queue can run without halting)."""
    key = (n, bool(with_nosoln))
    if key not in _period_cache:
        from util import mixed_cut, random_factor, stable_tau
        seq = PeriodSeq()
        seq.n, seq.kappa0 = n, 1.5
        seq.f = random_factor(n, 8100 + n)
        o = orc.OracleEllStable.new_with_matrix(seq.kappa0, seq.f, np.zeros(n))
        rng = np.random.default_rng(600 + n)
        seq.cuts, seq.status, seq.tsq, seq.snaps = [], [], [], {}
        for i in range(k):
            g = rng.standard_normal(n)
            g /= np.linalg.norm(g)
            sel = i if with_nosoln else (i // 7) * 8 + i % 7
            kind, b0, b1 = mixed_cut(sel, g, stable_tau(o, g), rng)
            seq.cuts.append((kind, g, b0, b1))
            seq.status.append(o.update(kind, g, b0, b1))
            seq.tsq.append(o.tsq)
            if i + 1 in PeriodSeq.SNAPS:
                seq.snaps[i + 1] = (o.mq.copy(), o.xc.copy(), o.kappa)
        _period_cache[key] = seq
    return _period_cache[key]


def oracle_from(orc, snap):
    mq, xc, kappa = snap
    return orc.OracleEllStable.new_with_matrix(kappa, mq.copy(), xc.copy())
