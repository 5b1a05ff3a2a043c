"""CPU reference of the batched low-pass design loop (include/ellhip_batch_lowpass.h): one oracle.OracleLowpass and one
OracleEll.new_with_scalar(40.0, zeros(n)) per instance, driven by the CPU oracle's own cutting_plane_optim /
cutting_plane_feas.  Finished runs are computed once per (n, constants, limits) and shared as read-only records; live
oracle / space pairs for the call-by-call and resume tests come from `fresh`."""
import functools

import numpy as np

from oracle import oracle as O

SUCCESS, NOSOLN, NOEFFECT, UNKNOWN = 0, 1, 2, 3
MAX_ITERS, TOL, KAPPA = 50000, 1e-14, 40.0
STATE_KEYS = ("more_alt", "idx1", "idx2", "idx3", "kmax", "nwpass", "nwstop", "fmax", "sp_sq")

CORRECTED = tuple(O.lowpass_case(True))
AS_WRITTEN = tuple(O.lowpass_case(False))
LOOSE = (0.12, 0.20, 0.5, 1.5, 0.3)
SHORT_PASSBAND = (0.02, 0.20, 0.5, 1.5, 0.3)      # n = 32: nwpass = 10 < n
EMPTY_TRANSITION = (0.15, 0.15, 0.5, 1.5, 0.3)
NO_STOPBAND_A = (1.0, 1.0, 0.5, 1.5, 0.3)
NO_STOPBAND_B = (0.5, 1.0, 0.5, 1.5, 0.3)
FEAS_INFEASIBLE = (0.12, 0.2, 0.9, 1.1, 1e-5)


def family(s):
    """the sweep of the tests and of tools/batch_lowpass_bench.py: band edges and ripple vary with s (period 6)"""
    wp = 0.08 + 0.01 * (s % 6)
    ws = wp + 0.08 + 0.01 * (s % 3)
    d = 0.02 + 0.01 * (s % 6)
    return (wp, ws, (1 - d) * (1 - d), (1 + d) * (1 + d), 0.1)


def fresh(n, consts):
    return O.OracleLowpass(n, *consts), O.OracleEll.new_with_scalar(KAPPA, np.zeros(n))


def space_record(space):
    return dict(mq=np.array(space.mq), xc=np.array(space.xc), kappa=space.kappa, tsq=space.tsq)


def _freeze(rec):
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def solve_optim(n, consts, max_iters=MAX_ITERS, tol=TOL, gamma=None):
    """cutting_plane_optim of one instance from a fresh oracle and space; gamma defaults to sp_sq"""
    omega, space = fresh(n, consts)
    x_best, niter, g, status = omega.cutting_plane_optim(space, consts[4] if gamma is None else gamma, max_iters, tol)
    return _freeze(dict(x_best=None if x_best is None else np.array(x_best), niter=niter, gamma=g, status=status,
                        state=omega.state(), **space_record(space)))


@functools.lru_cache(maxsize=None)
def solve_feas(n, consts, max_iters=MAX_ITERS, tol=TOL):
    omega, space = fresh(n, consts)
    x, niter, status = omega.cutting_plane_feas(space, max_iters, tol)
    return _freeze(dict(x_best=None if x is None else np.array(x), niter=niter, status=status, state=omega.state(),
                        **space_record(space)))


def columns(consts_list):
    """[(wpass, wstop, lp_sq, up_sq, sp_sq)] -> five [B] arrays"""
    return [np.array([c[k] for c in consts_list]) for k in range(5)]


def stack_state(states):
    return {k: np.array([s[k] for s in states]) for k in STATE_KEYS}
