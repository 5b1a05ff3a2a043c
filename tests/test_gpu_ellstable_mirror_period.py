"""The mirrored layout's periodic re-entry (STABLE_SOLVE = 3, the default form of every EllStable handle).

`ellstable_issue` leaves the layout and enters it again every ST_MIRROR_PERIOD = 256 updates so that the running row scales
stay products of few factors.  No other test keeps a handle inside the layout for more than 120 cuts, so none of this ran:
the leave + enter inside one ellhip_update and inside one queue_run, a failing cut as the last or the first update of a period,
the no-op updates of a halted queue crossing the boundary (the enter is refused on the device, the host still counts the
handle as mirrored until the results are read), and clones taken next to the boundary.  n = 64, 130, 257: one half, a ragged
second block, three chain blocks.  The 600-cut adaptive sequences come from the oracle alone and are shared by all tests
(tests/test_stable_step_check_cpu.py shows at least half of their cuts succeed).
"""
import numpy as np
import pytest

import stable_step_check as ssc
from util import TOL, assert_state_close, beta_of, rel_inf, set_default

pytestmark = pytest.mark.gpu
PERIOD = 256   # ST_MIRROR_PERIOD (csrc/ellstable_capi.inc.hpp)


def _handle(gpu, seq):
    set_default("STABLE_SOLVE", 3)
    h = gpu.EllStable.new_with_matrix(seq.kappa0, seq.f, np.zeros(seq.n))
    assert h.get_option(gpu.capi.OPT_STABLE_SOLVE) == 3
    return h


def _step(h, cut):
    kind, g, b0, b1 = cut
    return int(h._update(kind, (g, beta_of(b0, b1))))


def _fail_cut(seq, i):
    """Cut i's gradient with a bias no ellipsoid of this run reaches: NoSoln."""
    return (0, seq.cuts[i][1], 1e6, None)


def _bits_equal(a, b):
    return np.array_equal(a.mq, b.mq) and np.array_equal(a.xc(), b.xc()) and a.kappa == b.kappa and a.tsq() == b.tsq()


def _queue(h, cuts):
    kinds = np.array([c[0] for c in cuts], dtype=np.int32)
    grads = np.array([c[1] for c in cuts])
    b0 = np.array([c[2] for c in cuts], dtype=np.float64)
    b1 = np.array([np.nan if c[3] is None else c[3] for c in cuts], dtype=np.float64)
    h.queue_upload(kinds, grads, b0, b1)


def _close_to_snapshot(h, snap, what):
    mo, xo, ko = snap
    m = h.mq
    for name, part in (("factor", lambda a: np.triu(a, 1)), ("scratch", lambda a: np.tril(a, -1)), ("diagonal", np.diag)):
        assert rel_inf(part(m), part(mo)) <= TOL, f"{what}: {name}"
    assert rel_inf(h.xc(), xo) <= TOL and abs(h.kappa - ko) <= TOL * abs(ko), f"{what}: xc / kappa"


@pytest.mark.parametrize("n", ssc.PERIOD_SIZES)
def test_periodic_reentry_equals_an_observers_reentry(gpu, orc, n):
    """600 direct updates nobody observes (the layout is left and entered at updates 257 and 513, inside ellhip_update) against
    the same updates with the buffer read after updates 256 and 512.  An observer's leave followed by the next update's enter
    launches the same kernels on the same data as the periodic re-entry (k_st_mirror_leave, k_st_unscale_upper,
    k_st_mirror_clear; k_st_mirror_enter, k_st_mirror_mark), so the two handles are bit-identical by design -- buffer, xc,
    kappa and every tsq -- and both match the oracle.  Cut 255, the last update of the first period, is a NoSoln."""
    seq = ssc.period_sequence(orc, n, with_nosoln=True)
    a, b = _handle(gpu, seq), _handle(gpu, seq)
    seen = {}
    for i, cut in enumerate(seq.cuts):
        sa, sb = _step(a, cut), _step(b, cut)
        assert sa == sb == seq.status[i], (i, sa, sb, seq.status[i])
        assert a.tsq() == b.tsq(), i
        assert abs(a.tsq() - seq.tsq[i]) <= TOL * abs(seq.tsq[i]), i
        if i + 1 in (PERIOD, 2 * PERIOD):
            seen[i + 1] = b.mq
            assert b.get_option(gpu.capi.OPT_STABLE_MIRRORED) == 0 and a.get_option(gpu.capi.OPT_STABLE_MIRRORED) == 1
    assert sum(1 for s in seq.status if s == 0) >= len(seq.cuts) // 2
    assert _bits_equal(a, b)
    _close_to_snapshot(a, seq.snaps[600], f"n={n} after 600 cuts")
    _close_to_snapshot(b, seq.snaps[600], f"n={n} observed twin after 600 cuts")
    for k in (PERIOD, 2 * PERIOD):      # what the observer saw at the boundaries, scratch triangle included
        mo = seq.snaps[k][0]
        assert rel_inf(np.triu(seen[k]), np.triu(mo)) <= TOL and rel_inf(np.tril(seen[k], -1), np.tril(mo, -1)) <= TOL, k


@pytest.mark.parametrize("n", ssc.PERIOD_SIZES)
def test_queue_run_across_the_period(gpu, orc, n):
    """One queue_run of 300 cuts (the re-entry happens inside the call) and a twin that runs 256, has its buffer read and runs
    the other 44: per-cut tsq and status against the oracle, the two handles bit for bit."""
    seq = ssc.period_sequence(orc, n, with_nosoln=False)
    cuts = seq.cuts[:300]
    a, b = _handle(gpu, seq), _handle(gpu, seq)
    _queue(a, cuts)
    _queue(b, cuts)
    a.queue_run(0, 300)
    b.queue_run(0, PERIOD)
    mid = b.mq
    b.queue_run(PERIOD, 300 - PERIOD)
    for h in (a, b):
        st, ts = h.queue_results()
        assert list(st) == [0] * 300
        for i in range(300):
            assert abs(ts[i] - seq.tsq[i]) <= TOL * abs(seq.tsq[i]), i
    assert np.array_equal(a.queue_results()[1], b.queue_results()[1])
    assert _bits_equal(a, b)
    _close_to_snapshot(a, seq.snaps[300], f"n={n} queue of 300")
    assert rel_inf(np.triu(mid), np.triu(seq.snaps[PERIOD][0])) <= TOL


@pytest.mark.parametrize("at", [PERIOD, PERIOD + 1])
@pytest.mark.parametrize("n", ssc.PERIOD_SIZES)
def test_failing_cut_at_the_boundary(gpu, orc, n, at):
    """A NoSoln as update 256 (the last of a period) and as update 257 (the one that leaves and enters first), observed right
    after: the scratch triangle is the failing cut's; factor, diagonal, xc and kappa are, bit for bit, what a twin shows that
    stopped before the failing cut (observing the handle itself there would end the period early).  Successful cuts follow."""
    seq = ssc.period_sequence(orc, n, with_nosoln=False)
    y, x = _handle(gpu, seq), _handle(gpu, seq)
    for i in range(at - 1):
        assert _step(y, seq.cuts[i]) == _step(x, seq.cuts[i]) == 0
    o = ssc.oracle_from(orc, seq.snaps[at - 1])
    bad = _fail_cut(seq, at - 1)
    assert _step(y, bad) == o.update(bad[0], bad[1], bad[2], bad[3]) == 1
    my, mx = y.mq, x.mq
    assert np.array_equal(np.triu(my), np.triu(mx)) and np.array_equal(y.xc(), x.xc()) and y.kappa == x.kappa
    assert rel_inf(np.tril(my, -1), np.tril(o.mq, -1)) <= TOL            # the failing cut's scratch triangle
    assert abs(y.tsq() - o.tsq) <= TOL * abs(o.tsq)
    assert_state_close(y, o, what=f"n={n} failing cut as update {at}")
    for i in range(at - 1, at + 9):
        kind, g, b0, b1 = seq.cuts[i]
        assert _step(y, seq.cuts[i]) == o.update(kind, g, b0, b1) == 0
    assert_state_close(y, o, what=f"n={n} ten cuts after the failing update {at}")
    assert rel_inf(np.tril(y.mq, -1), np.tril(o.mq, -1)) <= TOL


@pytest.mark.parametrize("n", ssc.PERIOD_SIZES)
def test_halted_queue_across_the_boundary(gpu, orc, n):
    """A queue of 300 whose cut 250 fails: 49 no-op updates follow, and the one issued as update 257 leaves the layout (the
    failing cut's scratch triangle is built there) and is refused the enter on the device.  Reading the results gives the
    oracle's state after cut 250, and direct updates work afterwards (the second run on the halted queue: next test)."""
    seq = ssc.period_sequence(orc, n, with_nosoln=False)
    cuts = list(seq.cuts[:300])
    cuts[250] = _fail_cut(seq, 250)
    h = _handle(gpu, seq)
    _queue(h, cuts)
    h.queue_run(0, 300)
    st, ts = h.queue_results()
    assert list(st) == [0] * 250 + [1] + [3] * 49
    o = ssc.oracle_from(orc, seq.snaps[250])
    assert o.update(0, cuts[250][1], 1e6, None) == 1
    for i in range(250):
        assert abs(ts[i] - seq.tsq[i]) <= TOL * abs(seq.tsq[i]), i
    assert abs(ts[250] - o.tsq) <= TOL * abs(o.tsq)
    assert_state_close(h, o, what=f"n={n} after the halt")
    m1, x1, k1 = h.mq, h.xc(), h.kappa
    assert rel_inf(np.tril(m1, -1), np.tril(o.mq, -1)) <= TOL             # cut 250's scratch triangle
    assert rel_inf(np.triu(m1, 1), np.triu(o.mq, 1)) <= TOL and rel_inf(np.diag(m1), np.diag(o.mq)) <= TOL
    assert h.get_option(gpu.capi.OPT_STABLE_MIRRORED) == 0
    for i in range(251, 263):
        kind, g, b0, b1 = seq.cuts[i]
        assert _step(h, seq.cuts[i]) == o.update(kind, g, b0, b1) == 0
        assert abs(h.tsq() - o.tsq) <= TOL * abs(o.tsq), i
    assert h.get_option(gpu.capi.OPT_STABLE_MIRRORED) == 1
    assert_state_close(h, o, what=f"n={n} direct updates after the halt")
    assert rel_inf(np.tril(h.mq, -1), np.tril(o.mq, -1)) <= TOL


@pytest.mark.parametrize("n", ssc.PERIOD_SIZES)
def test_second_run_on_a_halted_queue_changes_nothing(gpu, orc, n):
    """The halted queue of the test above run in two calls, its results not read in between: the first stops at update 255
    (four no-ops behind the failing cut 250), the second issues the other 45 no-ops, the re-entry among them.  Buffer, xc, kappa
    and the recorded results are, bit for bit, those of a twin that ran the queue in one call; running the second range
    once more changes nothing either.  (A range that is run again on a halted queue has its slots marked 3, not run: the
    second call covers only cuts that had not been issued.)"""
    seq = ssc.period_sequence(orc, n, with_nosoln=False)
    cuts = list(seq.cuts[:300])
    cuts[250] = _fail_cut(seq, 250)
    a, b = _handle(gpu, seq), _handle(gpu, seq)
    _queue(a, cuts)
    _queue(b, cuts)
    a.queue_run(0, 300)
    b.queue_run(0, PERIOD - 1)
    b.queue_run(PERIOD - 1, 300 - (PERIOD - 1))
    b.queue_run(PERIOD - 1, 300 - (PERIOD - 1))
    assert np.array_equal(a.mq, b.mq) and np.array_equal(a.xc(), b.xc()) and a.kappa == b.kappa
    (sa, ta), (sb, tb) = a.queue_results(), b.queue_results()
    assert list(sa) == list(sb) == [0] * 250 + [1] + [3] * 49
    assert np.array_equal(ta[:251], tb[:251])
    assert np.array_equal(a.mq, b.mq)


@pytest.mark.parametrize("after", [PERIOD - 1, PERIOD])
@pytest.mark.parametrize("n", ssc.PERIOD_SIZES)
def test_clone_next_to_the_boundary(gpu, orc, n, after):
    """clone() after 255 and after 256 updates (it observes the source: the period starts again there); source and clone go
    on for ten cuts and both match the oracle."""
    seq = ssc.period_sequence(orc, n, with_nosoln=False)
    h = _handle(gpu, seq)
    for i in range(after):
        assert _step(h, seq.cuts[i]) == 0
    c = h.clone()
    o = ssc.oracle_from(orc, seq.snaps[after])
    _close_to_snapshot(c, seq.snaps[after], f"n={n} clone after {after}")
    for i in range(after, after + 10):
        kind, g, b0, b1 = seq.cuts[i]
        assert _step(h, seq.cuts[i]) == _step(c, seq.cuts[i]) == o.update(kind, g, b0, b1) == 0
    assert_state_close(h, o, what=f"n={n} source, ten cuts after the clone at {after}")
    assert_state_close(c, o, what=f"n={n} clone, ten cuts after {after}")
    assert rel_inf(np.triu(h.mq, 1), np.triu(o.mq, 1)) <= TOL and rel_inf(np.triu(c.mq, 1), np.triu(o.mq, 1)) <= TOL
