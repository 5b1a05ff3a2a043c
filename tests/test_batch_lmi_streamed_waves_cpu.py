"""CPU: the reference runs of tests/batch_lmi_streamed_wave_cases.py, which tests/test_gpu_batch_lmi_streamed_waves.py
compares the streamed LMI loops against at 4 to 16 waves, are pinned, and the set is checked for what it reaches INSIDE a
loop -- call 0 of every run is left out, since a run that is cut off after one call makes it too: 64-block pivots that
fail late, in the middle and early at 16 waves, a block cut, an objective cut and an all-pass round in one run, a feasible
exit after a late cut, a second 64-block that fails in its last row, nine stations walked and wrapped with J = 8, NoSoln
beside runs that go on.  So the GPU comparisons cannot pass vacuously, and a drifting reference is noticed before a GPU is
blamed."""
import pytest

import batch_lmi_streamed_wave_cases as waves

SUCCESS, NOSOLN = 0, 1
T = {t: i for i, t in enumerate(waves.cases.T_VALUES)}   # start t -> its member of a six-start batch

# (batch, EllStable?, feas?) -> per member (niter, status, has a point, idx afterwards)
PINS = {
    ('1024-64', False, False): [(30, 0, True, 1), (30, 0, True, 1), (30, 0, True, 0), (30, 0, False, 1), (30, 0, False, 0), (30, 0, False, 0)],
    ('1024-64', False, True): [(0, 0, True, 0), (0, 0, True, 0), (2, 0, True, 0), (30, 0, False, 0), (30, 0, False, 0), (30, 0, False, 0)],
    ('1024-64', True, False): [(30, 0, True, 1), (30, 0, True, 1), (30, 0, True, 0), (30, 0, False, 0), (30, 0, False, 0), (30, 0, False, 0)],
    ('1024-64', True, True): [(0, 0, True, 0), (0, 0, True, 0), (2, 0, True, 0), (30, 0, False, 0), (30, 0, False, 0), (30, 0, False, 0)],
    ('1023-64', False, False): [(12, 0, True, 1), (12, 0, True, 1), (12, 0, True, 1), (12, 0, False, 0), (12, 0, False, 0), (12, 0, False, 1)],
    ('1023-64', False, True): [(0, 0, True, 0), (0, 0, True, 0), (2, 0, True, 0), (12, 0, False, 0), (12, 0, False, 0), (12, 0, False, 0)],
    ('1023-64', True, False): [(12, 0, True, 1), (12, 0, True, 1), (12, 0, True, 1), (12, 0, False, 0), (12, 0, False, 0), (12, 0, False, 1)],
    ('1023-64', True, True): [(0, 0, True, 0), (0, 0, True, 0), (2, 0, True, 0), (12, 0, False, 0), (12, 0, False, 0), (12, 0, False, 0)],
    ('512-64x64', False, False): [(30, 0, True, 2), (30, 0, True, 1), (30, 0, True, 1), (30, 0, False, 0), (30, 0, False, 1), (30, 0, False, 2)],
    ('512-64x64', False, True): [(0, 0, True, 1), (0, 0, True, 1), (2, 0, True, 1), (30, 0, False, 1), (30, 0, False, 1), (30, 0, False, 1)],
    ('512-64x64', True, False): [(30, 0, True, 2), (30, 0, True, 1), (30, 0, True, 1), (30, 0, False, 0), (30, 0, False, 1), (30, 0, False, 2)],
    ('512-64x64', True, True): [(0, 0, True, 1), (0, 0, True, 1), (2, 0, True, 1), (30, 0, False, 1), (30, 0, False, 1), (30, 0, False, 1)],
    ('257-8..1', False, False): [(40, 0, True, 8), (40, 0, True, 6), (40, 0, True, 8), (40, 0, True, 2), (40, 0, True, 0), (40, 0, False, 1)],
    ('257-8..1', False, True): [(0, 0, True, 7), (0, 0, True, 7), (1, 0, True, 3), (11, 0, True, 2), (35, 0, True, 0), (40, 0, False, 3)],
    ('257-8..1', True, False): [(40, 0, True, 8), (40, 0, True, 6), (40, 0, True, 8), (40, 0, True, 2), (40, 0, True, 0), (40, 0, False, 4)],
    ('257-8..1', True, True): [(0, 0, True, 7), (0, 0, True, 7), (1, 0, True, 3), (11, 0, True, 2), (35, 0, True, 0), (40, 0, False, 2)],
    ('193-64x5', False, False): [(30, 0, True, 2), (30, 0, True, 2), (30, 0, True, 1), (30, 0, True, 2), (30, 0, True, 2), (30, 0, False, 0)],
    ('193-64x5', False, True): [(0, 0, True, 1), (0, 0, True, 1), (1, 0, True, 1), (2, 0, True, 1), (14, 0, True, 1), (30, 0, False, 1)],
    ('193-64x5', True, False): [(30, 0, True, 2), (30, 0, True, 2), (30, 0, True, 1), (30, 0, True, 1), (30, 0, True, 1), (30, 0, False, 0)],
    ('193-64x5', True, True): [(0, 0, True, 1), (0, 0, True, 1), (1, 0, True, 1), (2, 0, True, 1), (14, 0, True, 1), (30, 0, False, 1)],
    ('nosoln-1024', False, False): [(30, 0, False, 0), (30, 0, False, 1), (0, 1, False, 0)],
    ('nosoln-1024', False, True): [(30, 0, False, 0), (30, 0, False, 0), (0, 1, False, 0)],
    ('nosoln-1024', True, False): [(30, 0, False, 1), (30, 0, False, 1), (0, 1, False, 0)],
    ('nosoln-1024', True, True): [(30, 0, False, 0), (30, 0, False, 0), (0, 1, False, 0)],
}
PIN_KEYS = [(bid, stable, feas) for bid in waves.BATCH_IDS for stable in (False, True) for feas in (False, True)]
PIN_IDS = ["%s-%s-%s" % (b, "stable" if s else "ell", "feas" if f else "optim") for b, s, f in PIN_KEYS]
SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]


def summary(recs):
    return [(r["niter"], r["status"], r["x"] is not None, r["idx"]) for r in recs]


def in_loop(r):
    """(station, row) of every oracle call of a run but call 0"""
    return list(zip(r["stations"], r["rows"]))[1:]


def cut_rows(r, ms, size=None, block=None):
    """the failing rows of a run's in-loop block cuts, at blocks of `size` / at block `block`"""
    J = len(ms)
    return [row for st, row in in_loop(r) if st < J and (size is None or ms[st] == size) and (block is None or st == block)]


def test_the_pins_are_those_of_the_batches():
    assert sorted(PINS) == sorted(PIN_KEYS)
    for bid, (n, ms, who, max_iters, tol) in waves.BATCHES.items():
        assert 193 <= n <= 1024 and tol == 0.0 and all(len(PINS[(bid, s, f)]) == len(who) for s in (0, 1) for f in (0, 1))
        if not bid.startswith("nosoln"):
            assert who == waves.cases.members(n) and [w[1] for w in who] == list(waves.cases.T_VALUES)
    assert not set(waves.BATCHES) & set(waves.cases.BATCHES)   # beside the older batches, none of them replaced
    assert sorted({-(-waves.BATCHES[b][0] // 64) for b in waves.BATCHES}) == [4, 5, 8, 16]   # waves per workgroup
    assert waves.BATCHES["1023-64"][0] % 64 == 63 and waves.BATCHES["257-8..1"][0] % 64 == 1   # the last wave's live threads


@pytest.mark.parametrize("key", PIN_KEYS, ids=PIN_IDS)
def test_reference_pins(key):
    bid, stable, feas = key
    n, ms, who, max_iters, tol, recs = waves.batch_records(bid, stable, feas)
    assert summary(recs) == PINS[key]
    for r in recs:
        assert len(r["stations"]) == len(r["rows"]) and -1 <= r["idx"] <= len(ms)
        assert r["niter"] <= max_iters and r["mq"].size and r["xc"].shape == (n,)
        assert all(0 <= row < ms[st] for st, row in zip(r["stations"], r["rows"]) if st < len(ms))


@pytest.mark.parametrize("stable", SPACES)
def test_1024_64_fails_late_in_the_middle_and_early(stable):
    """the 64-block's failing rows inside the loops: >= 56 (the long witness solve, quadratic forms of p = 60-odd), several
    in 32 ... 55, some below 16; member t = 1.02 has every kind of round in one run and a feasible exit after a late cut"""
    ms = waves.BATCHES["1024-64"][1]
    J = len(ms)
    for feas in (False, True):
        recs = waves.batch_records("1024-64", stable, feas)[-1]
        rows = [cut_rows(r, ms, size=64) for r in recs]
        every = sorted({row for member in rows for row in member})
        assert any(row >= 56 for row in every) and any(row < 16 for row in every), every
        assert len([row for row in every if 32 <= row <= 55]) >= 4, every
        assert max(rows[T[1.02]]) >= 59, rows[T[1.02]]
        assert len({row for row in rows[T[1.5]] if 32 <= row <= 55}) >= 4, rows[T[1.5]]
        assert any(row < 16 for row in rows[T[6.0]]), rows[T[6.0]]
        late = recs[T[1.02]]
        if feas:   # the point is found at niter = 2, right after a cut at row 59
            assert late["niter"] == 2 and late["x"] is not None and late["status"] == SUCCESS
            assert in_loop(late) == [(0, 59), (J + 1, -1)]
        else:      # a block cut, an objective cut and a round that passes every station
            stations = {st for st, _ in in_loop(late)}
            assert stations == {0, J, J + 1}, stations
            assert {59, 61} <= set(cut_rows(late, ms, size=64))


@pytest.mark.parametrize("stable", SPACES)
def test_512_64x64_fails_in_the_last_row_of_the_second_block(stable):
    """block 1 fails at row 63 inside a loop, so block 0 was factorised through all 64 columns just before; and both blocks
    cut within one run, in the middle rows and in the first ones"""
    ms = waves.BATCHES["512-64x64"][1]
    recs = waves.batch_records("512-64x64", stable, False)[-1]
    assert any(63 in cut_rows(r, ms, block=1) for r in recs)
    both = [r for r in recs if cut_rows(r, ms, block=0) and cut_rows(r, ms, block=1)]
    assert len(both) >= 2
    for t, lo, hi in ((1.5, 37, 53), (6.0, 2, 13)):
        for feas in (False, True):
            r = waves.batch_records("512-64x64", stable, feas)[-1][T[t]]
            rows = cut_rows(r, ms, block=0) + cut_rows(r, ms, block=1)
            assert cut_rows(r, ms, block=0) and cut_rows(r, ms, block=1) and lo <= min(rows) and max(rows) <= hi, (t, rows)
    assert max(cut_rows(waves.batch_records("512-64x64", stable, True)[-1][T[1.5]], ms)) >= 52


@pytest.mark.parametrize("stable", SPACES)
def test_257_walks_and_wraps_nine_stations(stable):
    ms = waves.BATCHES["257-8..1"][1]
    J = len(ms)
    assert J == 8
    optim = waves.batch_records("257-8..1", stable, False)[-1]
    feas = waves.batch_records("257-8..1", stable, True)[-1]
    distinct = [len({st for st, _ in in_loop(r) if st < J}) for r in optim]
    assert max(distinct) >= 6 and distinct[T[6.0]] >= 6, distinct   # six blocks cut in one run
    assert any(r["idx"] == J for r in optim)                         # a run ends at the objective station
    assert any(len(r["stations"]) >= 9 for r in optim + feas)
    # the index wraps inside a loop: a cut at a lower station follows one at a higher station
    for r in (optim[T[6.0]], optim[T[3.0]], feas[T[3.0]]):
        sts = [st for st, _ in in_loop(r) if st <= J]
        assert sum(b < a for a, b in zip(sts, sts[1:])) >= 3, sts
    assert any(st == J for st, _ in in_loop(optim[T[6.0]]))          # an objective cut among them
    for t, niter in ((1.5, 11), (3.0, 35)):                          # `_feas` finds its point after a walk
        assert (feas[T[t]]["niter"], feas[T[t]]["x"] is not None) == (niter, True)
        assert in_loop(feas[T[t]])[-1] == (J + 1, -1)
    assert all(ms[st] - 1 >= row for r in optim for st, row in in_loop(r) if st < J)
    assert {row for r in optim for row in cut_rows(r, ms, size=8)} >= {3, 7}   # the 8-block's last row too


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("bid", ["1023-64", "193-64x5", "nosoln-1024"])
def test_the_other_batches_cut_at_a_64_block_inside_the_loop(bid, stable):
    ms = waves.BATCHES[bid][1]
    for feas in (False, True):
        recs = waves.batch_records(bid, stable, feas)[-1]
        assert any(cut_rows(r, ms, size=64) for r in recs), (bid, feas)
        if bid == "1023-64":   # late, with the thread that is not live
            assert max(row for r in recs for row in cut_rows(r, ms, size=64)) >= 56
        if bid == "nosoln-1024":
            status = [r["status"] for r in recs]
            assert NOSOLN in status and SUCCESS in status, status
            assert any(r["status"] == SUCCESS and r["niter"] == 30 for r in recs)   # a run that goes on beside it
