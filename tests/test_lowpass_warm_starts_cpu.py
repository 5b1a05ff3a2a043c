"""CPU: the warm starts of tests/lowpass_warm_starts.py do what the GPU tests of the streamed low-pass loops
(tests/test_gpu_batch_lowpass_streamed_warm.py) rely on.  These are conditions on the inputs, checked on the CPU loop alone, so
that the device comparisons cannot pass vacuously: within 30 rounds from new_with_scalar(KAPPA_WARM, x0) the six members reach
every return statement of assess_feas / assess_optim, shrink gamma repeatedly, end their `_feas` runs at round 0, late and
never, and visit thousands of table rows per oracle call where the runs from new_with_scalar(40, 0) visit 1.0 to 1.1.  The
runs are pinned (niter, status, the final gamma's bits, the calls per return statement), so a drifting reference is noticed
before a GPU is blamed."""
import collections
import functools

import numpy as np
import pytest

import batch_stable_loop_reference as ref
import lowpass_warm_starts as ws

ROUNDS = 30   # (the conditions are allowed 40)
SIZES = [193, 512, 1023]
SPACES = [False, True]

# per (n, stable) and member: the optim run (niter, status, gamma.hex(), calls per site in the order of ws.SITES), the feas run
# (niter, status, feasible, calls per site)
PINS = {
    (193, False): [
        ((30, 0, '0x1.00fdacb5453f4p-19', (0, 0, 9, 13, 0, 0, 8, 0)), (0, 0, True, (0, 0, 0, 0, 0, 0, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (30, 0, 0, 0, 0, 0, 0, 0)), (30, 0, False, (30, 0, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.b7fd70ff71c16p-5', (0, 0, 11, 0, 15, 0, 4, 0)), (15, 0, True, (0, 0, 0, 0, 15, 0, 0, 1))),
        ((30, 0, '0x1.0e1dadb330c97p-5', (0, 0, 28, 0, 0, 1, 1, 0)), (1, 0, True, (0, 0, 0, 0, 0, 1, 0, 1))),
        ((0, 1, '0x1.3333333333333p-2', (0, 1, 0, 0, 0, 0, 0, 0)), (0, 1, False, (0, 1, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.3333333333333p-2', (0, 0, 0, 30, 0, 0, 0, 0)), (30, 0, False, (0, 0, 0, 30, 0, 0, 0, 0))),
    ],
    (193, True): [
        ((30, 0, '0x1.ee76c706d9b6dp-20', (0, 0, 19, 0, 0, 0, 11, 0)), (0, 0, True, (0, 0, 0, 0, 0, 0, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (30, 0, 0, 0, 0, 0, 0, 0)), (30, 0, False, (30, 0, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.b8e634bc82e8bp-5', (0, 0, 10, 0, 16, 0, 4, 0)), (16, 0, True, (0, 0, 0, 0, 16, 0, 0, 1))),
        ((30, 0, '0x1.0e1dadb330c97p-5', (0, 0, 28, 0, 0, 1, 1, 0)), (1, 0, True, (0, 0, 0, 0, 0, 1, 0, 1))),
        ((0, 1, '0x1.3333333333333p-2', (0, 1, 0, 0, 0, 0, 0, 0)), (0, 1, False, (0, 1, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.3333333333333p-2', (0, 0, 0, 30, 0, 0, 0, 0)), (30, 0, False, (0, 0, 0, 30, 0, 0, 0, 0))),
    ],
    (512, False): [
        ((30, 0, '0x1.2859eac1c0bf4p-20', (0, 0, 15, 0, 0, 0, 15, 0)), (0, 0, True, (0, 0, 0, 0, 0, 0, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (30, 0, 0, 0, 0, 0, 0, 0)), (30, 0, False, (30, 0, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.a80aebcd21c0cp-5', (0, 0, 11, 0, 17, 0, 2, 0)), (17, 0, True, (0, 0, 0, 0, 17, 0, 0, 1))),
        ((30, 0, '0x1.193e0b92fd24ap-5', (0, 0, 28, 0, 0, 1, 1, 0)), (1, 0, True, (0, 0, 0, 0, 0, 1, 0, 1))),
        ((13, 1, '0x1.3333333333333p-2', (0, 14, 0, 0, 0, 0, 0, 0)), (13, 1, False, (0, 14, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.3333333333333p-2', (0, 0, 0, 30, 0, 0, 0, 0)), (30, 0, False, (0, 0, 0, 30, 0, 0, 0, 0))),
    ],
    (512, True): [
        ((30, 0, '0x1.4d5e9a7ca5b95p-20', (0, 0, 25, 0, 0, 0, 5, 0)), (0, 0, True, (0, 0, 0, 0, 0, 0, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (30, 0, 0, 0, 0, 0, 0, 0)), (30, 0, False, (30, 0, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.a7737a2f1bafap-5', (0, 0, 11, 0, 17, 0, 2, 0)), (17, 0, True, (0, 0, 0, 0, 17, 0, 0, 1))),
        ((30, 0, '0x1.193e0b92fd24ap-5', (0, 0, 28, 0, 0, 1, 1, 0)), (1, 0, True, (0, 0, 0, 0, 0, 1, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (0, 30, 0, 0, 0, 0, 0, 0)), (30, 0, False, (0, 30, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.3333333333333p-2', (0, 0, 0, 30, 0, 0, 0, 0)), (30, 0, False, (0, 0, 0, 30, 0, 0, 0, 0))),
    ],
    (1023, False): [
        ((30, 0, '0x1.22aa21d2880fcp-20', (0, 0, 25, 0, 0, 0, 5, 0)), (0, 0, True, (0, 0, 0, 0, 0, 0, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (30, 0, 0, 0, 0, 0, 0, 0)), (30, 0, False, (30, 0, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.a3308c6b00febp-5', (0, 0, 10, 0, 18, 0, 2, 0)), (18, 0, True, (0, 0, 0, 0, 18, 0, 0, 1))),
        ((30, 0, '0x1.1bf22dcd55157p-5', (0, 0, 28, 0, 0, 1, 1, 0)), (1, 0, True, (0, 0, 0, 0, 0, 1, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (0, 30, 0, 0, 0, 0, 0, 0)), (30, 0, False, (0, 30, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.3333333333333p-2', (0, 0, 0, 30, 0, 0, 0, 0)), (30, 0, False, (0, 0, 0, 30, 0, 0, 0, 0))),
    ],
    (1023, True): [
        ((30, 0, '0x1.28b3542250e31p-20', (0, 0, 28, 0, 0, 0, 2, 0)), (0, 0, True, (0, 0, 0, 0, 0, 0, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (30, 0, 0, 0, 0, 0, 0, 0)), (30, 0, False, (30, 0, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.a2e28c9201af9p-5', (0, 0, 10, 0, 18, 0, 2, 0)), (18, 0, True, (0, 0, 0, 0, 18, 0, 0, 1))),
        ((30, 0, '0x1.1bf22dcd55157p-5', (0, 0, 28, 0, 0, 1, 1, 0)), (1, 0, True, (0, 0, 0, 0, 0, 1, 0, 1))),
        ((30, 0, '0x1.3333333333333p-2', (0, 30, 0, 0, 0, 0, 0, 0)), (30, 0, False, (0, 30, 0, 0, 0, 0, 0, 0))),
        ((30, 0, '0x1.3333333333333p-2', (0, 0, 0, 30, 0, 0, 0, 0)), (30, 0, False, (0, 0, 0, 30, 0, 0, 0, 0))),
    ],
}


@functools.lru_cache(maxsize=None)
def traces(n, stable):
    """-> [(optim trace, feas trace)] of the six members"""
    return [(ws.trace(n, c, x0, stable, ROUNDS), ws.trace(n, c, x0, stable, ROUNDS, feas=True)) for c, x0 in ws.starts(n)]


def counts(sites):
    c = collections.Counter(sites)
    return tuple(c[s] for s in ws.SITES)


both = pytest.mark.parametrize("stable", SPACES, ids=["Ell", "EllStable"])
sizes = pytest.mark.parametrize("n", SIZES)


@sizes
@both
def test_pins(n, stable):
    for m, ((t, f), (want_t, want_f)) in enumerate(zip(traces(n, stable), PINS[n, stable])):
        assert (t["niter"], t["status"], float(t["gamma"]).hex(), counts(t["sites"])) == want_t, ws.MEMBERS[m]
        assert (f["niter"], f["status"], f["x_best"] is not None, counts(f["sites"])) == want_f, ws.MEMBERS[m]


@sizes
@both
def test_every_return_site_is_reached(n, stable):
    reached = collections.Counter()
    for t, f in traces(n, stable):
        reached.update(t["sites"])
        reached.update(f["sites"])
    assert all(reached[s] >= 1 for s in ws.SITES), {s: reached[s] for s in ws.SITES}
    optim = collections.Counter(s for t, _ in traces(n, stable) for s in t["sites"])   # and all but `feasible` inside optim runs
    assert all(optim[s] >= 1 for s in ws.SITES if s != ws.FEASIBLE) and optim[ws.FEASIBLE] == 0


@sizes
@both
def test_two_members_shrink_twice_and_go_on(n, stable):
    """two or more shrunk rounds, each followed by a further cut: the CENTRAL update of a shrunk cut succeeded, and the
    state it left was cut again"""
    often = 0
    for t, _ in traces(n, stable):
        at = [k for k, s in enumerate(t["sites"]) if s == ws.SHRUNK and k + 1 < len(t["sites"])]
        if len(at) >= 2:
            often += 1
            assert t["x_best"] is not None and t["gamma"] < ws.LOOSE[4]
    assert often >= 2


@sizes
@both
def test_feas_runs_end_at_once_late_and_never(n, stable):
    f = [f for _, f in traces(n, stable)]
    assert (f[0]["niter"], f[0]["status"], f[0]["sites"]) == (0, ref.SUCCESS, [ws.FEASIBLE])
    assert f[2]["niter"] >= 1 and f[2]["status"] == ref.SUCCESS and f[2]["sites"][-1] == ws.FEASIBLE
    assert len(f[2]["sites"]) == f[2]["niter"] + 1 and f[2]["x_best"] is not None
    assert (f[1]["niter"], f[1]["status"], f[1]["x_best"]) == (ROUNDS, ref.SUCCESS, None)
    assert ws.FEASIBLE not in f[1]["sites"]


@sizes
@both
def test_rows_visited_per_call(n, stable):
    rows = [r for t, f in traces(n, stable) for r in t["rows"] + f["rows"]]
    assert np.mean(rows) > 2.0
    assert np.mean(rows) > 500.0   # (in fact: 700 to 3100)
    cold = ws.trace(n, ws.LOOSE, np.zeros(n), stable, ROUNDS, kappa=40.0)   # the start of the other tests of these loops
    assert set(cold["sites"]) <= {ws.PASS_LOW, ws.PASS_HIGH} and np.mean(cold["rows"]) < 0.05 * np.mean(rows)


@sizes
@both
def test_the_hand_stepped_loop_is_the_cpu_loop(n, stable):
    """ws.trace against cutting_plane_optim / cutting_plane_feas from the same starts: the records the GPU tests compare with"""
    for feas in (False, True):
        recs = ws.warm_records(n, stable, feas, ROUNDS)
        for m, (r, pair) in enumerate(zip(recs, traces(n, stable))):
            t = pair[feas]
            assert (r["niter"], r["status"], r["x_best"] is not None) == (t["niter"], t["status"], t["x_best"] is not None), m
            assert r["state"] == t["state"] and r["tsq"] == t["tsq"] and r["kappa"] == t["kappa"]
            assert np.array_equal(r["xc"], t["xc"]) and np.array_equal(r["mq"], t["mq"])
            assert feas or r["gamma"] == t["gamma"]
            assert r["x_best"] is None or np.array_equal(r["x_best"], t["x_best"])


def test_return_site_rejects_a_wrong_cut():
    """the classifier checks what it names: a cut with another row's gradient or a shifted beta is no return of the oracle"""
    n = 193
    c, x0 = ws.starts(n)[2]
    omega = ws.O.OracleLowpass(n, *c)
    before = omega.state()
    g, (b0, b1) = omega.assess_feas(x0)
    after = omega.state()
    assert ws.return_site(omega, x0, (g, (b0, b1)), before, after)[0] == ws.TRANSITION_NEGATIVE
    with pytest.raises(AssertionError):
        ws.return_site(omega, x0, (g, (np.nextafter(b0, 1.0), b1)), before, after)
    with pytest.raises(AssertionError):
        ws.return_site(omega, x0, (-omega.spectrum[after["idx2"] - 1], (b0, b1)), before, after)
