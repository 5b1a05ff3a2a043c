"""CPU reference of the batched SVM loop (include/ellhip_batch_svm.h): one svm_reference.cutting_plane_optim per instance
over oracle.OracleEll.new_with_scalar(100.0, zeros(n)), gamma = +inf at the start.  The space is handed to the loop behind
a thin recorder so that the CutStatus of the last update is known as well.  Finished runs of the test family are computed
once per (s, m, nfeat, max_iters, tol) and shared as read-only records; `run` drives any table, labels and space."""
import functools

import numpy as np

import svm_reference as svm
from oracle import oracle as O

SUCCESS, NOSOLN, NOEFFECT, UNKNOWN = 0, 1, 2, 3
KAPPA = 100.0
SHIFTS = (1.0, 0.2, 0.45)
# (m, nfeat, tol, max_iters) and niter of the members s = 0..5
ROWS = (
    (64, 2, 1e-12, 2000, (2, 277, 257, 3, 281, 73)),
    (96, 7, 1e-8, 3000, (6, 1439, 1233, 4, 1436, 143)),
    (257, 15, 1e-6, 4000, (12, 4000, 4000, 12, 4000, 420)),
)


def clouds(m, nfeat, shift, seed):
    """two clouds around +-shift on feature 0, labels -1 for every third sample, +1 otherwise (as tests/test_gpu_svm.py)"""
    rng = np.random.default_rng(seed)
    lab = np.where(np.arange(m) % 3 == 0, -1, 1).astype(np.int32)
    X = rng.random((m, nfeat)) - 0.5
    X[:, 0] += shift * lab
    return X, lab


def family(s, m, nfeat):
    """member s: separable for s % 3 == 0 (ends on the zero cut), overlapping otherwise"""
    return clouds(m, nfeat, SHIFTS[s % 3], s)


class Recorder:
    """what svm_reference.cutting_plane_optim needs of a space, plus the status of the last update"""

    def __init__(self, space):
        self.space, self.status = space, SUCCESS

    @property
    def xc(self):
        return self.space.xc

    @property
    def tsq(self):
        return self.space.tsq

    def update_central_cut(self, g, beta):
        self.status = self.space.update_central_cut(g, beta)
        return self.status


def fresh(n):
    return O.OracleEll.new_with_scalar(KAPPA, np.zeros(n))


def space_record(space):
    return dict(mq=np.array(space.mq), xc=np.array(space.xc), kappa=space.kappa, tsq=space.tsq)


def run(data, labels, max_iters, tol, space=None, gamma=np.inf, last=(0, np.inf)):
    """cutting_plane_optim of one instance on `space` (fresh when None): a record of everything the loop leaves.  last:
    the oracle's (min_idx, min_val) before the call, kept when no iteration runs."""
    data = np.asarray(data, dtype=np.float64)
    space = fresh(data.shape[1] + 1) if space is None else space
    rec = Recorder(space)
    x_best, niter, gamma, chosen = svm.cutting_plane_optim(data, labels, rec, gamma, max_iters, tol)
    if x_best is not None:  # the last scan looked at x_best
        last = svm.argmin(svm.margins(data, labels, x_best))
        assert last[0] == chosen[-1]
    return dict(x_best=x_best, niter=niter, gamma=gamma, status=rec.status, min_idx=last[0], min_val=last[1],
                **space_record(space))


def _freeze(rec):
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def solve(s, m, nfeat, max_iters, tol):
    """member s of the family from a fresh space"""
    X, lab = family(s, m, nfeat)
    return _freeze(run(X, lab, max_iters, tol))
