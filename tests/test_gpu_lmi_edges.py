"""GPU: the device LDLTMgr / LMIOracle / LMI0Oracle (include/ellhip_lmi.h) past the sizes a CPU factor can follow,
and at the edges of its kernels: every accumulator slot of k_lmi_witness, the 32-row panel and 256-column forming
slab boundaries, partial last panels, a reused handle, zero / tiny / non-finite pivots, the row chunks of k_lmi_quad.

No CPU-oracle factor above m = 1057.  Above it the device is judged by tests/lmi_cases.py: matrices whose LDL' is
known in closed form and exact in fp64 (bit-for-bit comparison), matrices whose failing row is certain by
construction with residual bounds derived from u = 2^-53, and single-entry F_k for which g is a known answer that
does not depend on the order of any sum.  Each check prints its worst residual / bound (`LMI_EDGE ...`; run with -s)."""
import numpy as np
import pytest

import lmi_cases as lc

pytestmark = pytest.mark.gpu

TINY = -2.0 ** -40


def note(what, value):
    print(f"LMI_EDGE {what} {value:.3g}")


# ------------------------------------------------------------------------------------------- exact factor at scale

# (m, what, 0-based pivot).  289 = 9 * 32 + 1, 2081 = 65 * 32 + 1, 7201 = 225 * 32 + 1: the last panel is one row
# wide; 7201 reaches the 29th forming slab (columns 7168 ...).  The mid pivots sit on either side of a slab boundary.
EXACT_CASES = [(m, what, k) for m, mid0, mid1 in ((289, 256, 255), (2081, 1023, 1024), (7201, 7168, 7167))
               for what, k in (("spd", None), ("zero", mid0), ("zero", m - 1), ("tiny", mid1), ("tiny", m - 1))]
EXACT_CASES.append((7201, "tiny", 3071))  # -2^-40 itself at m = 7201: see tiny_value


@pytest.fixture(scope="module")
def pencils():
    """one ExactPencil per m, built at first use and shared by that m's cases; dropped with the module"""
    cache = {}
    yield lambda m: cache[m] if m in cache else cache.setdefault(m, lc.ExactPencil(m, np.random.default_rng(m)))
    cache.clear()


def tiny_value(ex, k):
    """-2^-40 wherever c[k-1] - 2^-40 is an fp64 number (c[k-1] < 2^13, rows up to about 4000); past that the
    closed form is exact only for a coarser pivot and -2^-38 is used (representable for every c < 2^15 > 4 m).
    ExactPencil.case raises if the value it is given is not exact at that row."""
    return TINY if k == 0 or ex.c[k - 1] < 2.0 ** 13 else 4.0 * TINY


@pytest.mark.parametrize("m,what,k", EXACT_CASES)
def test_exact_factor_at_scale(gpu, pencils, m, what, k):
    ex = pencils(m)
    value = {"spd": None, "zero": 0.0, "tiny": None if k is None else tiny_value(ex, k)}[what]
    if (m, k) == (7201, 3071):
        assert value == TINY
    case = ex.case(k, value if value is not None else 0.0)
    dev = gpu.LDLTMgr(m)
    assert dev.factorize(case[0]) == (k is None)
    storage = dev.storage
    lc.check_exact(storage, dev.pos, None if k is None else dev.witness(), case)
    if k is None:
        if m <= 2081:
            np.testing.assert_array_equal(dev.sqrt(), lc.expected_sqrt(storage))
        return
    # the witness of this family is a known answer too: L[i][j] = s_i / s_j gives v = e_k - (s_k / s_{k-1}) e_{k-1},
    # every partial sum of the back substitution being exact
    v = np.zeros(m)
    v[k] = 1.0
    if k:
        v[k - 1] = -ex.s[k] / ex.s[k - 1]
    np.testing.assert_array_equal(dev.wit, v)


# ------------------------------------------------------------------------------------------- every witness slot

# the smallest sizes whose owner slot (p - 2) >> 10 reaches 1, 2 and 7; (7201, 7169) ends on slot 7's first column
WITNESS_CASES = [(1057, 1057), (1057, 1025), (2081, 2081), (7201, 7201), (7201, 7169)]


@pytest.mark.parametrize("m,p", WITNESS_CASES)
def test_every_witness_slot(gpu, orc, m, p):
    """F(x) = 1.0 * F_0 + 0.0 * F_1 with F_0 = generic_pencil (fails at row p for certain) and F_1 dense (so that
    every row chunk of k_lmi_quad carries weight in g[1], lmi_cases.second_matrix)."""
    rng = np.random.default_rng(10000 * m + p)
    F = np.empty((2, m, m))
    F[0] = lc.generic_pencil(m, p, rng)
    F[1] = lc.second_matrix(m, rng)
    x = np.array([1.0, 0.0])
    dev = gpu.LMI0Oracle(F)
    cut = dev.assess_feas(x)
    assert cut is not None and dev.pos == (0, p)
    g, ep = cut
    storage, v = dev.storage, dev.wit
    assert (p - 2) >> 10 == {1057: 1, 1025: 0, 2081: 2, 7201: 7, 7169: 6}[p]
    z = rng.standard_normal((p, 3 if p <= lc.LONGDOUBLE_MAX_P else 1))
    note(f"witness m={m} p={p}", lc.check_witness(storage, v, p))
    note(f"factor_probe m={m} p={p}", lc.check_factor_probe(F[0], storage, p, z))
    note(f"ep m={m} p={p}", lc.check_ep(F[0], storage, v, p, ep))
    note(f"quad_F0 m={m} p={p}", lc.check_quad(F[0], v, p, g[0], -1.0))
    note(f"quad_F1 m={m} p={p}", lc.check_quad(F[1], v, p, g[1], -1.0))
    if m > 1057:
        return
    cpu = orc.OracleLMI(F)
    gc, epc = cpu.assess_feas(x)
    assert cpu.ldlt.pos == (0, p)
    np.testing.assert_array_equal(storage[:p, :p], cpu.ldlt.storage[:p, :p])
    assert ep == epc
    wc = cpu.ldlt.wit[:p]
    assert np.allclose(v[:p], wc, rtol=1e-11, atol=1e-13 * np.max(np.abs(wc)))


# ------------------------------------------------------------------------------------------- one reused handle

SWEEP_Q = [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 258, 287, 288, 289, 290, 160]
SWEEP_SEED = 3


def sweep_order(qs):
    """the seeded shuffle of the walk; it must hold a late failure (last panels, second forming slab) directly
    followed by an early one (first panel), so that the early call runs over the late call's leftovers"""
    order = [int(i) for i in np.random.default_rng(SWEEP_SEED).permutation(len(SWEEP_Q)) if SWEEP_Q[i] in qs]
    seq = [SWEEP_Q[i] for i in order]
    assert any(a >= 287 and b <= 2 for a, b in zip(seq, seq[1:])), seq
    return [qs.index(q) for q in seq]


def single_entry_pencil(m, qs, seed):
    """B positive definite as in test_gpu_lmi.random_pencil; F_k = e_q e_q' for q = qs[k] (1-based); t with
    B - t e_q e_q' failing exactly at row q: rows before q see B alone, and the pivot at q is at most
    B[q][q] - t <= lambda_max(B) - t < 0."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, m))
    B = a @ a.T / m + np.eye(m)
    B = (B + B.T) / 2.0
    F = np.zeros((len(qs), m, m))
    for k, q in enumerate(qs):
        F[k, q - 1, q - 1] = 1.0
    return F, B, 2.0 * float(np.linalg.eigvalsh(B)[-1]) + 1.0


def walk(gpu, orc, m, qs, order, lmi0, feasible_every=3):
    """One device handle and one CPU oracle through failing rows qs[k], k in `order`, with a feasible call after
    every third one.  LMIOracle: F(x) = B - sum x_k F_k, x = t e_k.  LMI0Oracle: B rides as F_0 with x_0 = 1 and
    x = -t e_k (the same F(x), element for element).

    After each call pos, storage[:p, :p] and ep equal the CPU oracle's bit for bit, and g is a known answer:
    v'(e_q e_q')v has one nonzero term, so g[j] == sign * wit[q_j - 1]**2 exactly however k_lmi_quad splits and
    reduces its rows -- 1.0 for the failing row itself, 0.0 for every q_j > p."""
    F, B, t = single_entry_pencil(m, qs, seed=m)
    n = len(qs)
    if lmi0:
        F = np.concatenate([B[None], F])
        dev, cpu, sign, off = gpu.LMI0Oracle(F), orc.OracleLMI(F), -1.0, 1
    else:
        dev, cpu, sign, off = gpu.LMIOracle(F, B), orc.OracleLMI(F, B), 1.0, 0
    rows = np.array(qs) - 1
    worst = 0.0
    for step, k in enumerate(order):
        p = qs[k]
        x = np.zeros(n + off)
        if lmi0:
            x[0], x[1 + k] = 1.0, -t
        else:
            x[k] = t
        rd, rc = dev.assess_feas(x), cpu.assess_feas(x)
        assert rd is not None and rc is not None and dev.pos == cpu.ldlt.pos == (0, p), (step, p, dev.pos)
        np.testing.assert_array_equal(dev.storage[:p, :p], cpu.ldlt.storage[:p, :p])
        g, ep = rd[0], (rd[1] if lmi0 else rd[1].beta)
        assert ep == rc[1] and np.signbit(ep) == np.signbit(rc[1])
        v = dev.wit
        assert v[p - 1] == 1.0 and not np.any(v[p:])
        assert g[off + k] == sign * 1.0
        np.testing.assert_array_equal(g[off:], sign * v[rows] ** 2)
        assert np.allclose(v[:p], cpu.ldlt.wit[:p], rtol=1e-11, atol=1e-13 * np.max(np.abs(cpu.ldlt.wit[:p])))
        if lmi0:
            worst = max(worst, lc.check_quad(B, v, p, g[0], -1.0))
        if (step + 1) % feasible_every == 0:
            x = np.zeros(n + off)
            if lmi0:
                x[0] = 1.0
            assert dev.assess_feas(x) is None and cpu.assess_feas(x) is None
            assert dev.pos == cpu.ldlt.pos == (0, 0)
            np.testing.assert_array_equal(dev.storage, cpu.ldlt.storage)
    return worst


@pytest.mark.parametrize("m", [290, 288])
def test_pivot_sweep_on_one_reused_handle(gpu, orc, m):
    """m = 290: the last panel is 2 rows wide (rows 288, 289) and follows a full one; m = 288: the last panel is
    full and has no trailing update.  Pivots on both sides of every panel boundary up to 64, of the slab boundary
    at 256, in a last panel of width 1 (q = 289 is its first row, 290 its last) and 31 rows into a panel (q = 32,
    64, 288)."""
    qs = [q for q in SWEEP_Q if q <= m]
    walk(gpu, orc, m, qs, sweep_order(qs), lmi0=False)


def test_pivot_sweep_lmi0(gpu, orc):
    note("quad_B sweep m=290", walk(gpu, orc, 290, SWEEP_Q, sweep_order(SWEEP_Q), lmi0=True))


def test_small_p_through_the_chunk_split(gpu, orc):
    """rows_per = ceil(p / 8) of k_lmi_quad: p = 1, 2, 7 leave chunks empty, p = 8 fills each with one row, p = 9
    leaves the last three empty.  The handle first fails at the very last row, then at the small ones."""
    qs = [290, 1, 2, 7, 8, 9]
    for lmi0 in (False, True):
        walk(gpu, orc, 290, qs, [0, 5, 1, 4, 2, 3, 0, 3], lmi0=lmi0)


# ------------------------------------------------------------------------------------------- non-finite input

def same_as_cpu(dev, cpu, x, m):
    rd, rc = dev.assess_feas(x), cpu.assess_feas(x)
    assert (rd is None) == (rc is None)
    assert dev.pos == cpu.ldlt.pos
    rows = m if dev.pos[1] == 0 else dev.pos[1]
    np.testing.assert_array_equal(dev.storage[:rows, :rows], cpu.ldlt.storage[:rows, :rows])  # NaN == NaN here
    if rc is not None:
        np.testing.assert_array_equal(rd[1].beta, rc[1])
        finite = np.isfinite(rc[0])
        np.testing.assert_array_equal(rd[0][~finite], rc[0][~finite])
        scale = np.max(np.abs(rc[0][finite]), initial=0.0)
        assert np.all(np.abs(rd[0][finite] - rc[0][finite]) <= 1e-10 * scale)
    return rc is not None


@pytest.mark.parametrize("m", [33, 257])
def test_non_finite_input_follows_the_reference(gpu, orc, m):
    """A NaN pivot is "not <= 0.0": the reference goes on and reports SPD.  The device makes the same comparison;
    and a handle that has seen NaN / inf answers the next finite x like a fresh one."""
    n = 3
    rng = np.random.default_rng(m)
    a = rng.standard_normal((m, m))
    B = a @ a.T / m + np.eye(m)
    F = rng.standard_normal((n, m, m))
    F = (F + F.transpose(0, 2, 1)) / 2.0
    x_feas, x_cut = np.zeros(n), np.array([0.4, -0.3, 0.5])
    dev, cpu = gpu.LMIOracle(F, B), orc.OracleLMI(F, B)
    assert same_as_cpu(dev, cpu, x_cut, m) and not same_as_cpu(dev, cpu, x_feas, m)
    for bad in (np.array([0.1, np.nan, 0.2]), np.array([0.1, np.inf, -0.2]), np.array([-np.inf, 0.0, 0.1])):
        same_as_cpu(dev, cpu, bad, m)
        assert same_as_cpu(dev, cpu, x_cut, m)
        same_as_cpu(dev, cpu, bad, m)
        assert not same_as_cpu(dev, cpu, x_feas, m)
    assert not same_as_cpu(dev, cpu, np.array([np.nan, 0.0, 0.0]), m) and np.all(np.isnan(dev.storage))
    Bn = B.copy()
    Bn[m // 2, m // 2] = np.nan
    dev, cpu = gpu.LMIOracle(F, Bn), orc.OracleLMI(F, Bn)
    assert not same_as_cpu(dev, cpu, x_feas, m) and np.isnan(dev.storage[m // 2, m // 2])
    same_as_cpu(dev, cpu, x_cut, m)
    assert not same_as_cpu(dev, cpu, x_feas, m)
