"""What the GPU tests of the batched max-cut loops share (tests/test_gpu_batch_maxcut*.py): batches of the test family,
the four kinds of batch handle, exact comparisons of a device run with CPU records (tests/batch_maxcut_reference.py), and
the host-driven form of the loop -- one ellhip_batch_maxcut_assess_optim and one ellhip_batch_update per iteration.

Every comparison is EXACT: float64 bit patterns (the sign of a zero counts; NaN is compared by position) and integers."""
import numpy as np

import batch_maxcut_reference as ref

INF = np.inf


def same_bits(a, b):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def assert_bits(got, want, what):
    assert same_bits(got, want), (what, got, want)


def lds_epw(n):
    """instances per workgroup of the LDS engine's Ell loop (include/ellhip_batch.h)"""
    epw = min(64, (256 if n <= 64 else 128) // n)
    while epw > 1 and epw * 8 * ((n * (n | 1) + 2 * n + 8) | 1) > 64 * 1024:
        epw -= 1
    return epw


class Batch:
    """B problems: tables [B][n][n] (or one [n][n] when shared) and starting centres [B][n]"""

    def __init__(self, tables, xc0, shared=False, kappa=ref.KAPPA):
        self.tables, self.xc0, self.shared, self.kappa = np.asarray(tables, dtype=np.float64), np.asarray(xc0), shared, kappa
        self.B, self.n = self.xc0.shape

    def table(self, b):
        return self.tables if self.shared else self.tables[b]

    def problem(self, gpu):
        return gpu.BatchMaxcutProblem(self.tables, self.B, shared=self.shared)

    def spaces(self, gpu, stable, streamed):
        cls = {(False, True): gpu.EllBatchStreamed, (True, True): gpu.EllStableBatchStreamed,
               (False, False): gpu.EllBatch, (True, False): gpu.EllStableBatch}[(stable, streamed)]
        batch = cls.new_with_scalar(np.full(self.B, self.kappa), self.xc0)
        assert bool(getattr(batch, "is_streamed", False)) == streamed
        assert batch.variant == (gpu.capi.SPACE_ELL_STABLE if stable else gpu.capi.SPACE_ELL)
        return batch

    def cpu_spaces(self, stable):
        return [ref.fresh(self.xc0[b], stable, self.kappa) for b in range(self.B)]

    def cpu_runs(self, stable, max_iters, tol=ref.TOL, spaces=None, gamma=None):
        spaces = self.cpu_spaces(stable) if spaces is None else spaces
        gamma = np.full(self.B, -INF) if gamma is None else gamma
        return [ref.run(self.table(b), max_iters, tol, spaces[b], gamma[b]) for b in range(self.B)]


def family_batch(n, B, shared=False):
    """members 0 .. B-1, "mixed" and "pos" interleaved so that neighbours stop at different rounds; shared: member 0's
    table from every member's starting centre"""
    sets = [ref.weights(s, n, "mixed" if s % 2 == 0 else "pos") for s in range(B)]
    xc0 = np.stack([x for _, x in sets])
    return Batch(sets[0][0] if shared else np.stack([w for w, _ in sets]), xc0, shared)


def assert_runs_equal(got, recs, n):
    x_best, has, niter, gamma, status = got
    np.testing.assert_array_equal(niter, np.array([r["niter"] for r in recs], dtype=np.int64))
    np.testing.assert_array_equal(status, np.array([r["status"] for r in recs], dtype=np.int32))
    np.testing.assert_array_equal(has, np.array([r["x_best"] is not None for r in recs], dtype=np.int32))
    assert_bits(gamma, np.array([r["gamma"] for r in recs]), "gamma")
    want = np.stack([np.full(n, np.nan) if r["x_best"] is None else r["x_best"] for r in recs])
    assert_bits(x_best, want, "x_best")   # rows without a result stay as the caller left them (NaN)


def assert_state_equal(batch, recs):
    """the spaces afterwards; on EllStable `mq` is the packed buffer with its scratch triangle"""
    assert_bits(batch.mq, np.stack([r["mq"] for r in recs]), "mq")
    assert_bits(batch.xc(), np.stack([r["xc"] for r in recs]), "xc")
    assert_bits(batch.kappa, np.array([r["kappa"] for r in recs]), "kappa")
    assert_bits(batch.tsq(), np.array([r["tsq"] for r in recs]), "tsq")


def device_records(got, batch):
    """a device run as records of the CPU reference's shape, for comparing two device runs with each other"""
    x_best, has, niter, gamma, status = got
    mq, xc, kappa, tsq = batch.mq, batch.xc(), batch.kappa, batch.tsq()
    return [dict(x_best=x_best[b] if has[b] else None, niter=int(niter[b]), gamma=gamma[b], status=int(status[b]),
                 mq=mq[b], xc=xc[b], kappa=kappa[b], tsq=tsq[b]) for b in range(len(has))]


def check_loop(gpu, case, stable, streamed, recs, max_iters, tol=ref.TOL, chunk=None):
    prob = case.problem(gpu)
    if chunk is not None:
        prob.set_chunk(chunk)
    batch = case.spaces(gpu, stable, streamed)
    got = prob.optim(batch, -INF, max_iters, tol)
    assert_runs_equal(got, recs, case.n)
    assert_state_equal(batch, recs)
    return prob, batch, got


def host_driven(prob, batch, max_iters, tol=ref.TOL):
    """The loop of every instance with both halves on the device but the host in between: one wide assess_optim and one
    ellhip_batch_update (K = 1) per iteration.  The batch is updated as a whole, so an instance that has stopped is handed a
    cut that fails (NoSoln) from then on; its state is read back at the moment it stops, and the records hold those
    snapshots."""
    B, n = prob.B, prob.n
    rec = [None] * B
    x_best = [None] * B
    gamma = np.full(B, -INF)
    for it in range(max_iters):
        live = [b for b in range(B) if rec[b] is None]
        if not live:
            break
        xc = batch.xc()
        grad, beta, shrunk, gamma_new, _ = prob.assess_optim(xc, gamma)
        kinds = np.zeros(B, dtype=np.int32)
        grads = np.zeros((B, n))
        grads[:, 0] = 1.0
        b0 = np.full(B, 1e300)  # a bias cut with beta > tau: NoSoln
        for b in live:
            gamma[b] = gamma_new[b]
            if shrunk[b]:
                x_best[b] = xc[b].copy()
            kinds[b], grads[b], b0[b] = (1 if shrunk[b] else 0), grad[b], beta[b]
        st, tsq = batch.update(kinds, grads, b0)
        ended = [b for b in live if st[0, b] != ref.SUCCESS or tsq[0, b] < tol]
        if it == max_iters - 1:
            ended = live
        if ended:
            mq, xcs, kappa, tsqs = batch.mq, batch.xc(), batch.kappa, batch.tsq()
            for b in ended:
                stopped = st[0, b] != ref.SUCCESS or tsq[0, b] < tol
                rec[b] = dict(x_best=x_best[b], niter=it if stopped else max_iters, gamma=gamma[b],
                              status=int(st[0, b]) if stopped else ref.SUCCESS, mq=mq[b].copy(), xc=xcs[b].copy(),
                              kappa=kappa[b], tsq=tsqs[b])
    return rec
