"""Expected values for the batched device-resident loops on EllStable batch handles
(include/ellhip_batch_stable_loops.h).  No new CPU arithmetic: the loops are the existing helpers
(batch_lmi_reference.optim / feas, OracleLowpass.cutting_plane_optim / cutting_plane_feas, batch_svm_reference.run) handed
oracle.OracleEllStable spaces.

A `Case` is one batch of problems of one kind with a start state per instance.  `cpu_run` gives one record per instance of
everything the CPU loop leaves; `host_driven` gives the same records from the host-driven form on the device -- the CPU
oracle per instance and ellhip_batch_update with K = 1 on the EllStable batch, a host round trip per iteration -- which is
an independent second check of the device loop."""
import ctypes as C
import math

import numpy as np

import batch_lmi_reference as lmi
import batch_lowpass_reference as lp
import batch_svm_reference as bsvm
import svm_reference as svm
from oracle import oracle as O
from util import random_factor

SUCCESS, NOSOLN, NOEFFECT, UNKNOWN = 0, 1, 2, 3
BIAS, CENTRAL = 0, 1
KINDS = ("lmi_optim", "lmi_feas", "lp_optim", "lp_feas", "svm")


class Case:
    """kind: one of KINDS.  problems: per instance (fs, bs, c) for LMI, the five constants for low-pass, (data, labels)
    for SVM.  kappa [B], xc [B][n]; mq [B][n][n] or None (None: EllStable::new_with_scalar(kappa, xc)).  shared: the SVM
    instances use problems[0]'s table."""

    def __init__(self, kind, problems, n, kappa, xc, mq=None, *, max_iters, tol, gamma=None, use_parallel=True,
                 shared=False):
        assert kind in KINDS
        self.kind, self.problems, self.n, self.B = kind, list(problems), int(n), len(problems)
        self.kappa = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (self.B,)).copy()
        self.xc = np.broadcast_to(np.asarray(xc, dtype=np.float64), (self.B, self.n)).copy()
        self.mq = None if mq is None else np.asarray(mq, dtype=np.float64)
        self.max_iters, self.tol, self.use_parallel, self.shared = int(max_iters), float(tol), use_parallel, shared
        if gamma is None:
            gamma = [p[4] for p in self.problems] if kind == "lp_optim" else math.inf
        self.gamma = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)).copy()

    @property
    def optim(self):
        return self.kind in ("lmi_optim", "lp_optim", "svm")

    def with_random_factors(self, seed):
        """the same problems from EllStable::new_with_matrix states: a random factor, junk in the scratch triangle"""
        rng = np.random.default_rng(seed)
        self.kappa = 0.5 * self.kappa + rng.random(self.B)
        self.mq = np.stack([random_factor(self.n, int(rng.integers(1 << 30))) for _ in range(self.B)])
        return self


def set_use_parallel_cut(space, flag):
    """orc_ellstable has no setter for its EllCalc's flag: set it through the head of the struct (oracle/ell_oracle.h)"""
    class Head(C.Structure):
        _fields_ = [("n", C.c_int64), ("mq", C.c_void_p), ("xc", C.c_void_p), ("kappa", C.c_double), ("tsq", C.c_double),
                    ("corrected", C.c_int), ("helper", O._Calc)]
    C.cast(C.c_void_p(space.h), C.POINTER(Head)).contents.helper.use_parallel_cut = int(flag)


def cpu_space(case, b):
    if case.mq is None:
        s = O.OracleEllStable.new_with_scalar(case.kappa[b], case.xc[b])
    else:
        s = O.OracleEllStable.new_with_matrix(case.kappa[b], case.mq[b], case.xc[b])
    if not case.use_parallel:
        set_use_parallel_cut(s, 0)
    return s


def space_record(space):
    return dict(mq=np.array(space.mq), xc=np.array(space.xc), kappa=space.kappa, tsq=space.tsq)


def _oracle(case, b):
    p = case.problems[b]
    if case.kind == "lmi_optim":
        return lmi.RoundRobinLmi(p[0], p[1], p[2])
    if case.kind == "lmi_feas":
        return lmi.RoundRobinLmi(p[0], p[1], None)
    if case.kind in ("lp_optim", "lp_feas"):
        return O.OracleLowpass(case.n, *p)
    return None


def _oracle_state(case, omega, last=None):
    if case.kind.startswith("lmi"):
        return dict(idx=omega.idx)
    if case.kind.startswith("lp"):
        return omega.state()
    return dict(min_idx=last[0], min_val=last[1])


def cpu_run(case):
    """the CPU loop of every instance -> [dict(x_best, niter, gamma, status, state, mq, xc, kappa, tsq)]"""
    out = []
    for b in range(case.B):
        space, omega = cpu_space(case, b), _oracle(case, b)
        gamma = case.gamma[b]
        if case.kind == "lmi_optim":
            x, niter, gamma, status = lmi.optim(space, omega, gamma, case.max_iters, case.tol)
        elif case.kind == "lmi_feas":
            x, niter, status = lmi.feas(space, omega, case.max_iters, case.tol)
        elif case.kind == "lp_optim":
            x, niter, gamma, status = omega.cutting_plane_optim(space, gamma, case.max_iters, case.tol)
        elif case.kind == "lp_feas":
            x, niter, status = omega.cutting_plane_feas(space, case.max_iters, case.tol)
        else:
            data, lab = svm_table(case, b)
            r = bsvm.run(data, lab, case.max_iters, case.tol, space=space, gamma=gamma)
            out.append(dict(x_best=r["x_best"], niter=r["niter"], gamma=r["gamma"], status=r["status"],
                            state=dict(min_idx=r["min_idx"], min_val=r["min_val"]), **space_record(space)))
            continue
        out.append(dict(x_best=None if x is None else np.array(x), niter=niter, gamma=gamma, status=status,
                        state=_oracle_state(case, omega), **space_record(space)))
    return out


def svm_table(case, b):
    return (case.problems[0][0] if case.shared else case.problems[b][0]), case.problems[b][1]


class Stepper:
    """One oracle call of instance b for the host-driven form: step(x, gamma) -> (what, kind, g, b0, b1, gamma) with
    what in {"cut", "best" (a cut, and x is the best point so far), "found" (feasible: the loop ends), "error"}."""

    def __init__(self, case, b):
        self.case, self.b, self.omega, self.last = case, b, _oracle(case, b), (0, math.inf)

    def step(self, x, gamma):
        k = self.case.kind
        if k == "lmi_optim":
            (g, beta), station, gamma = self.omega.assess_optim(x, gamma)
            best = station == self.omega.J + 1
            return ("best" if best else "cut"), (CENTRAL if best else BIAS), g, beta, None, gamma
        if k in ("lmi_feas", "lp_feas"):
            cut = self.omega.assess_feas(x)
            if cut is None:
                return "found", BIAS, None, 0.0, None, gamma
            if k == "lmi_feas":
                (g, beta), _ = cut
                return "cut", BIAS, g, beta, None, gamma
            g, (b0, b1) = cut
            return "cut", BIAS, g, b0, b1, gamma
        if k == "lp_optim":
            try:
                (g, (b0, b1)), shrunk, gamma = self.omega.assess_optim(x, gamma)
            except IndexError:  # a feasible point without a stopband maximum: the reference panics, the loops answer Unknown
                return "error", BIAS, None, 0.0, None, gamma
            return ("best" if shrunk else "cut"), (CENTRAL if shrunk else BIAS), g, b0, b1, gamma
        data, lab = svm_table(self.case, self.b)
        (g, beta), _, gamma, idx, val = svm.assess_optim(data, lab, x)
        self.last = (idx, val)
        return "best", CENTRAL, g, beta, None, gamma

    def state(self):
        return _oracle_state(self.case, self.omega, self.last)


def host_driven(batch, case):
    """The loop of every instance with the update on the device, one ellhip_batch_update (K = 1) per iteration.  The batch
    is updated as a whole, so an instance that has stopped is handed a cut that fails (NoSoln) from then on; its state is
    read back at the moment it stops, and the records hold those snapshots."""
    B, n = case.B, case.n
    steps = [Stepper(case, b) for b in range(B)]
    rec = [None] * B
    x_best = [None] * B
    gamma = case.gamma.copy()
    niter = [case.max_iters] * B
    status = [SUCCESS] * B

    def snapshot(which):
        if not which:
            return
        mq, xc, kappa, tsq = batch.mq, batch.xc(), batch.kappa, batch.tsq()
        for b in which:
            rec[b] = dict(x_best=x_best[b], niter=niter[b], gamma=gamma[b], status=status[b], state=steps[b].state(),
                          mq=mq[b].copy(), xc=xc[b].copy(), kappa=kappa[b], tsq=tsq[b])

    for it in range(case.max_iters):
        live = [b for b in range(B) if rec[b] is None]
        if not live:
            break
        xc = batch.xc()
        kinds = np.zeros(B, dtype=np.int32)
        grads = np.zeros((B, n))
        grads[:, 0] = 1.0
        b0 = np.full(B, 1e300)  # a bias cut with beta > tau: NoSoln
        b1 = np.full(B, np.nan)
        ended, acted = [], []
        for b in live:
            what, kind, g, c0, c1, gamma[b] = steps[b].step(xc[b].copy(), gamma[b])
            if what in ("found", "error"):
                if what == "found":
                    x_best[b] = xc[b].copy()
                niter[b], status[b] = it, (SUCCESS if what == "found" else UNKNOWN)
                ended.append(b)
                continue
            if what == "best":
                x_best[b] = xc[b].copy()
            kinds[b], grads[b], b0[b] = kind, g, c0
            if c1 is not None:
                b1[b] = c1
            acted.append(b)
        snapshot(ended)  # before the update: the cut parked on them touches tsq and the scratch triangle
        st, tsq = batch.update(kinds, grads, b0, b1)
        ended = []
        for b in acted:
            if st[0, b] != SUCCESS or tsq[0, b] < case.tol:
                niter[b], status[b] = it, int(st[0, b])
                ended.append(b)
        snapshot(ended)
    snapshot([b for b in range(B) if rec[b] is None])
    return rec


# ---- the inputs of the tests ------------------------------------------------------------------------------------------
def lmi_case(problems, *, feas=False, kappa=10.0, xc=None, max_iters=2000, tol=1e-8):
    n = len(problems[0][2])
    return Case("lmi_feas" if feas else "lmi_optim", problems, n, kappa, np.zeros(n) if xc is None else xc,
                max_iters=max_iters, tol=tol)


def lmi_feas_case(problems):
    """EllStable::new_with_scalar(40, 3 N(0, 1)) centres from default_rng(5)"""
    n = len(problems[0][2])
    xc = 3.0 * np.random.default_rng(5).standard_normal((len(problems), n))
    return lmi_case(problems, feas=True, kappa=40.0, xc=xc, tol=1e-8)


def lp_case(n, consts, *, feas=False, max_iters=1500, tol=lp.TOL, use_parallel=True):
    return Case("lp_feas" if feas else "lp_optim", [tuple(c) for c in consts], n, lp.KAPPA, np.zeros(n),
                max_iters=max_iters, tol=tol, use_parallel=use_parallel)


def svm_case(m, nfeat, tol, members, *, shared=False, max_iters=1500):
    problems = [bsvm.family(s, m, nfeat) for s in members]
    if shared:  # one table, labels flipped differently per instance
        X, lab = problems[0]
        problems = []
        for s in members:
            flip = np.random.default_rng(40 + s).random(m) < 0.02 * (s % 3)
            problems.append((X, np.where(flip, -lab, lab).astype(np.int32)))
    return Case("svm", problems, nfeat + 1, bsvm.KAPPA, np.zeros(nfeat + 1), max_iters=max_iters, tol=tol, shared=shared)
