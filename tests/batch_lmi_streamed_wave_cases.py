"""Batches of the LMI loops on streamed batch handles at 4 to 16 waves, shared by
tests/test_batch_lmi_streamed_waves_cpu.py and tests/test_gpu_batch_lmi_streamed_waves.py.

The problems, starts and CPU runs are those of tests/batch_lmi_streamed_cases.py, unchanged; its BATCHES has one shape above
three waves, (1024; 64, 7) over 8 rounds, in which the 64-block never fails past row 20.  These batches run long enough, and
with the 64-block as the tight block, for the factorisation to stop late in a 64-block inside the loop (a long witness solve,
quadratic forms of p = 60-odd), for a second 64-block to fail after a first was fully factorised, for the round-robin index
to walk and wrap over nine stations, and for NoSoln beside a run that goes on, at 4, 5, 8 and 16 waves and with a thread that
is not live in the last wave."""
import batch_lmi_streamed_cases as cases

KF = cases.KF
SIX = cases.members(0)   # the six starts T_VALUES over seeds 0, 1, 2

# id -> (n, ms, who, max_iters, tol); who: (seed, t[, kf])
BATCHES = {
    "1024-64": (1024, (64,), SIX, 30, 0.0),                       # 16 waves, the 64-block is the tight block
    "1023-64": (1023, (64,), SIX, 12, 0.0),                       # a thread that is not live in wave 16
    "512-64x64": (512, (64, 64), SIX, 30, 0.0),                   # 8 waves; 64 columns factorised, then a block that fails
    "257-8..1": (257, (8, 7, 6, 5, 4, 3, 2, 1), SIX, 40, 0.0),    # 5 waves, one live thread in the last; J = 8
    "193-64x5": (193, (64, 5), SIX, 30, 0.0),                     # 4 waves
    "nosoln-1024": (1024, (64,), ((0, 3.0, 0.01), (1, 1.5, KF), (0, 6.0, 1e-4)), 30, 0.0),   # NoSoln beside a run that goes on
}
BATCH_IDS = list(BATCHES)


def batch_records(bid, stable, feas):
    """-> (n, ms, who, max_iters, tol, records) of a batch on one space and one loop (cached and read-only, cases.record)"""
    n, ms, who, max_iters, tol = BATCHES[bid]
    recs = [cases.record(stable, feas, w[0], n, ms, w[1], w[2] if len(w) > 2 else KF, max_iters, tol) for w in who]
    return n, ms, who, max_iters, tol, recs
