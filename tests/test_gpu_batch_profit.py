"""GPU: the batched device-resident profit loops (include/ellhip_batch_profit.h) -- cutting_plane_optim over ProfitOracle and
ProfitRbOracle, cutting_plane_optim_q over ProfitOracleQ, on Ell and EllStable batch handles -- against the reference's
oracles and drivers restated in tests/batch_profit_reference.py with the library's own exp and log.  Host and device run the
same roundings, so every comparison is EXACT (float64 bit patterns, integers): niter, status, has_best, gamma, x_best and the
spaces afterwards (mq -- on EllStable the packed buffer with its scratch triangle -- xc, kappa, tsq)."""
import ctypes as C

import numpy as np
import pytest

import batch_maxcut_checks as chk
import batch_profit_reference as ref

pytestmark = pytest.mark.gpu

SPACES = [pytest.param(False, id="ell"), pytest.param(True, id="stable")]
KINDS = [pytest.param(k, id=name) for name, k in ref.KINDS.items()]


def problem(gpu, kind, B):
    params, a, v, vparams, _ = ref.family()
    return gpu.BatchProfitProblem(kind, params[:B], a[:B], v[:B], vparams[:B] if kind == ref.ROBUST else None)


def spaces(gpu, stable, B):
    cls = gpu.EllStableBatch if stable else gpu.EllBatch
    return cls.new_with_scalar(np.full(B, ref.KAPPA), ref.family()[4][:B])


def loop(prob, batch, gamma, max_iters=ref.MAX_ITERS, tol=ref.TOL):
    return (prob.optim_q if prob.kind == ref.DISCRETE else prob.optim)(batch, gamma, max_iters, tol)


def check_loop(gpu, kind, stable, B, chunk=None):
    recs = [ref.solve(kind, b, stable) for b in range(B)]
    prob, batch = problem(gpu, kind, B), spaces(gpu, stable, B)
    if chunk is not None:
        prob.set_chunk(chunk)
    got = loop(prob, batch, 0.0)
    chk.assert_runs_equal(got, recs, 2)
    chk.assert_state_equal(batch, recs)
    return recs


# ---- ell_exp / ell_log on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["exp", "log"])
def test_math_on_the_device(gpu, fn):
    xs = np.concatenate([ref.math_sweep(fn), ref.EXP_SPECIALS if fn == "exp" else ref.LOG_SPECIALS])
    got = gpu.math_eval(fn, xs)
    want = ref.host_eval(fn, xs)
    assert chk.same_bits(got, want), np.nonzero(got.view(np.int64) != want.view(np.int64))[0][:10]


# ---- the reference's pins -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_pins(gpu, kind):
    """src/oracles/profit_oracle.rs:172-225 through the device loops: Ell::new([100, 100], 0), gamma = 0, default options"""
    vp = np.array([ref.PIN_VPARAMS]) if kind == ref.ROBUST else None
    prob = gpu.BatchProfitProblem(kind, np.array([ref.PIN_PARAMS]), np.array([ref.PIN_A]), np.array([ref.PIN_V]), vp)
    batch = gpu.EllBatch.new(np.full((1, 2), 100.0), np.zeros((1, 2)))
    got = loop(prob, batch, 0.0)
    assert got[2][0] == ref.PINS[kind] and got[1][0] == 1 and got[0][0, 0] <= np.log(30.5)
    rec = ref.pin_run(kind)
    chk.assert_runs_equal(got, [rec], 2)
    chk.assert_state_equal(batch, [rec])


# ---- bit-identity with the CPU reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [200, 1, 65])
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("kind", KINDS)
def test_loop_against_the_cpu_runs(gpu, kind, stable, B):
    """B = 200: three full workgroups of 64 and one of 8; 65: one full and one with a single problem"""
    recs = check_loop(gpu, kind, stable, B)
    if B == 200 and kind == ref.DISCRETE:   # the retry path and NoEffect are among what was compared
        assert sum(r["retries"] > 0 for r in recs) >= 2 and sum(r["status"] == ref.NOEFFECT for r in recs) >= 2


@pytest.mark.parametrize("chunk", [1, 7])
@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("kind", KINDS)
def test_chunks_give_the_same_bits(gpu, kind, stable, chunk):
    """launches of 1 and of 7 rounds (the default, 256, is every other test): the cursor, yd and retry cross launches -- with
    chunk = 1 every NoEffect and its retry are in different launches"""
    check_loop(gpu, kind, stable, ref.FAMILY_B, chunk)


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_second_call_continues(gpu, kind, stable):
    """max_iters = 10, then a second call: the reference run the same way with the same oracle object"""
    B = ref.FAMILY_B
    xc0 = ref.family()[4]
    oracles = [ref.family_oracle(kind, b) for b in range(B)]
    cpu = [ref.fresh(xc0[b], stable) for b in range(B)]
    first = [ref.run(kind, oracles[b], cpu[b], 0.0, 10) for b in range(B)]
    assert all(r["niter"] == 10 for r in first)
    prob, batch = problem(gpu, kind, B), spaces(gpu, stable, B)
    got = loop(prob, batch, 0.0, 10)
    chk.assert_runs_equal(got, first, 2)
    chk.assert_state_equal(batch, first)
    second = [ref.run(kind, oracles[b], cpu[b], first[b]["gamma"]) for b in range(B)]
    got = loop(prob, batch, got[3])
    chk.assert_runs_equal(got, second, 2)
    chk.assert_state_equal(batch, second)


# ---- the wide calls and the host-driven loop ----------------------------------------------------------------------------------
def host_driven(prob, batch, oracles, max_iters=ref.MAX_ITERS, tol=ref.TOL):
    """The loop with both halves on the device but the host in between: one wide assess and one ellhip_batch_update (K = 1)
    per iteration, each wide call compared with the reference oracles' own.  The batch is updated as a whole, so a problem
    that has stopped is handed a cut that fails (NoSoln) from then on; its state is read back at the moment it stops."""
    B, q = prob.B, prob.kind == ref.DISCRETE
    rec, x_best = [None] * B, [None] * B
    gamma, retry = np.zeros(B), np.zeros(B, dtype=np.int32)
    for it in range(max_iters):
        live = [b for b in range(B) if rec[b] is None]
        if not live:
            break
        xc = batch.xc()
        if q:
            grad, beta, shrunk, x_q, more, gamma_new = prob.assess_optim_q(xc, gamma, retry)
        else:
            grad, beta, shrunk, gamma_new = prob.assess_optim(xc, gamma)
            x_q, more = xc, np.ones(B, dtype=bool)
        for b in live:   # the wide call against the reference's, per call
            if q:
                (g, bt), sh, xq, ma, gm = oracles[b].assess_optim_q([float(xc[b, 0]), float(xc[b, 1])], gamma[b], bool(retry[b]))
                assert chk.same_bits(x_q[b], xq) and bool(more[b]) == ma, (it, b)
            else:
                (g, bt), sh, gm = oracles[b].assess_optim([float(xc[b, 0]), float(xc[b, 1])], gamma[b])
            assert chk.same_bits(grad[b], g) and chk.same_bits(beta[b], bt) and chk.same_bits(gamma_new[b], gm), (it, b)
            assert bool(shrunk[b]) == sh, (it, b)
        kinds = np.full(B, 2 if q else 0, dtype=np.int32)
        grads = np.zeros((B, 2))
        grads[:, 0] = 1.0
        b0 = np.full(B, 1e300)   # beta > tau: NoSoln, the space untouched
        for b in live:
            gamma[b] = gamma_new[b]
            if shrunk[b]:
                x_best[b] = x_q[b].copy()
                retry[b] = 0
            kinds[b] = 2 if q else (1 if shrunk[b] else 0)
            grads[b], b0[b] = grad[b], beta[b]
        st, tsq = batch.update(kinds, grads, b0)
        ended = {}
        for b in live:
            s = int(st[0, b])
            if not q:
                if s != ref.SUCCESS or tsq[0, b] < tol:
                    ended[b] = (it, s)
                continue
            if s == ref.SUCCESS:
                retry[b] = 0
            if s == ref.NOSOLN or (s == ref.NOEFFECT and not more[b]):
                ended[b] = (it, s)
                continue
            if s == ref.NOEFFECT:
                retry[b] = 1
            if tsq[0, b] < tol:
                ended[b] = (it, ref.SUCCESS)
        if it == max_iters - 1:
            for b in live:
                ended.setdefault(b, (max_iters, ref.SUCCESS))
        if ended:
            mq, xcs, kappa, tsqs = batch.mq, batch.xc(), batch.kappa, batch.tsq()
            for b, (niter, status) in ended.items():
                rec[b] = dict(x_best=x_best[b], niter=niter, gamma=gamma[b], status=status, mq=mq[b].copy(), xc=xcs[b].copy(),
                              kappa=kappa[b], tsq=tsqs[b])
    return rec


@pytest.mark.parametrize("stable", SPACES)
@pytest.mark.parametrize("kind", KINDS)
def test_wide_calls_and_the_host_driven_loop(gpu, kind, stable):
    B = ref.FAMILY_B
    prob, batch = problem(gpu, kind, B), spaces(gpu, stable, B)
    got = loop(prob, batch, 0.0)
    other = spaces(gpu, stable, B)
    recs = host_driven(problem(gpu, kind, B), other, [ref.family_oracle(kind, b) for b in range(B)])
    chk.assert_runs_equal(got, recs, 2)
    chk.assert_state_equal(batch, recs)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(gpu):
    lib = gpu.capi.load()
    B = 5
    probs = {k: problem(gpu, k, B) for k in (ref.PLAIN, ref.ROBUST, ref.DISCRETE)}
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = np.random.default_rng(2)

    def refused(entry, batch, oracle, text=None):
        before = (batch.mq, batch.xc(), batch.kappa, batch.tsq())
        gamma = np.full(oracle.B, 0.3)
        xb = np.full((oracle.B, 2), np.nan)
        has = np.full(oracle.B, -5, dtype=np.int32)
        niter = np.full(oracle.B, -5, dtype=np.int64)
        status = np.full(oracle.B, -5, dtype=np.int32)
        rc = getattr(lib, entry)(batch._h, oracle._h, ptr(gamma), 100, 1e-10, ptr(xb), ptr(has), ptr(niter), ptr(status))
        assert rc == gpu.capi.E_INVALID and lib.ellhip_last_error(), entry
        if text:
            assert text in lib.ellhip_last_error(), (entry, lib.ellhip_last_error())
        for a, b in zip(before, (batch.mq, batch.xc(), batch.kappa, batch.tsq())):
            assert chk.same_bits(a, b)
        assert np.isnan(xb).all() and (gamma == 0.3).all()
        assert (has == -5).all() and (niter == -5).all() and (status == -5).all()

    def make(cls, B=B, n=2):
        return cls.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, n)))

    ell, stb = make(gpu.EllBatch), make(gpu.EllStableBatch)
    plain, disc = "ellhip_batch_profit_optim", "ellhip_batch_profit_optim_q"
    for entry, oracle in ((plain, probs[ref.PLAIN]), (plain, probs[ref.ROBUST]), (disc, probs[ref.DISCRETE])):
        refused(entry, stb, oracle)                                        # the wrong variant
        refused(entry + "_stable", ell, oracle)
        refused(entry, make(gpu.EllBatch, n=3), oracle, b"n = 2")          # n != 2
        refused(entry + "_stable", make(gpu.EllStableBatch, n=1), oracle, b"n = 2")
        refused(entry, make(gpu.EllBatch, B=B + 1), oracle)                # B differs
        refused(entry, make(gpu.EllBatchStreamed), oracle, b"streamed")    # streamed handles
        refused(entry + "_stable", make(gpu.EllStableBatchStreamed), oracle, b"streamed")
    for batch, suffix in ((ell, ""), (stb, "_stable")):                    # the wrong kind for the entry point
        refused(disc + suffix, batch, probs[ref.PLAIN], b"discrete")
        refused(disc + suffix, batch, probs[ref.ROBUST], b"discrete")
        refused(plain + suffix, batch, probs[ref.DISCRETE], b"discrete")
    x = np.zeros((B, 2))
    with pytest.raises(gpu.capi.EllHipError):
        probs[ref.DISCRETE].assess_optim(x, 0.0)
    with pytest.raises(gpu.capi.EllHipError):
        probs[ref.PLAIN].assess_optim_q(x, 0.0, 0)
    with pytest.raises(gpu.capi.EllHipError):
        probs[ref.PLAIN].set_chunk(0)
    with pytest.raises(ValueError):
        probs[ref.PLAIN].assess_optim(np.zeros((B, 3)), 0.0)
    if lib.ellhip_device_count() > 1:
        refused(plain, gpu.EllBatch.new_with_scalar(np.full(B, 10.0), rng.standard_normal((B, 2)), device=1), probs[ref.PLAIN])
    # and the good pairs still run
    for kind in (ref.PLAIN, ref.ROBUST, ref.DISCRETE):
        check_loop(gpu, kind, False, B)
