"""GPU: all 20 entry points of the batched device-resident loops (LMI and low-pass optim / feas, SVM optim; each on the
LDS engine and on the streamed engine, with Ell and with EllStable spaces) against the four kinds of batch handle.

With the handle kind it is made for, an entry point called through the raw symbol returns, to the bit, what the Python
mirror's optim / feas returns from the same start: the mirror's choice of entry point and the symbol agree.  With each of the
other three kinds, with a wrong B or n, with a NULL argument and (LMI) with a handle made for the other of optim / feas, it
returns E_INVALID, ellhip_last_error() holds the text written out below, and the outputs keep their fill.  The texts are
the library's as read from its source, not computed by it; where two checks would both refuse, the earlier one speaks
(NULL, then LMI's c, then the handle kind, then B and n).  Refusals launch nothing.

B = 2 and the n of the existing refusal tests' constructors: 3 (LMI family A), 8 (low-pass), nfeat = 2 (SVM)."""
import ctypes as C
import math

import numpy as np
import pytest

import batch_lmi_reference as lmi
import batch_lowpass_reference as lp
import batch_stable_loop_reference as ref

pytestmark = pytest.mark.gpu

B, ROUNDS = 2, 3
KINDS = ("lds", "lds_stable", "streamed", "streamed_stable")
ENGINE_OF_KIND = {"lds": "", "lds_stable": "_stable", "streamed": "_streamed", "streamed_stable": "_streamed_stable"}

# (oracle, engine suffix) -> what a refusal calls the loop
WHAT = {
    ("lmi", ""): "batched LMI loop",
    ("lmi", "_stable"): "batched LMI loop",
    ("lmi", "_streamed"): "batched LMI streamed loop",
    ("lmi", "_streamed_stable"): "batched LMI streamed EllStable loop",
    ("lowpass", ""): "batched lowpass loop",
    ("lowpass", "_stable"): "batched lowpass loop",
    ("lowpass", "_streamed"): "batched lowpass streamed loop",
    ("lowpass", "_streamed_stable"): "batched lowpass streamed EllStable loop",
    ("svm", ""): "batched svm loop",
    ("svm", "_stable"): "batched svm loop",
    ("svm", "_streamed"): "batched svm streamed loop",
    ("svm", "_streamed_stable"): "batched svm streamed EllStable loop",
}
# (engine suffix, kind of the handle it is given) -> the rest of the refusal
WRONG_KIND = {
    ("", "lds_stable"): ": EllStable batch handles are not supported",
    ("", "streamed"): ": streamed batch handles are not supported",
    ("", "streamed_stable"): ": streamed batch handles are not supported",
    ("_stable", "lds"): ": the _stable entry points take EllStable batch handles only",
    ("_stable", "streamed"): ": streamed batch handles are not supported",
    ("_stable", "streamed_stable"): ": streamed batch handles are not supported",
    ("_streamed", "lds"): ": the _streamed entry points take streamed batch handles only",
    ("_streamed", "lds_stable"): ": the _streamed entry points take streamed batch handles only",
    ("_streamed", "streamed_stable"): ": EllStable batch handles are not supported",
    ("_streamed_stable", "lds"): ": the _streamed_stable entry points take streamed batch handles only",
    ("_streamed_stable", "lds_stable"): ": the _streamed_stable entry points take streamed batch handles only",
    ("_streamed_stable", "streamed"): ": the _streamed_stable entry points take EllStable batch handles only",
}
WRONG_SHAPE = {
    "lmi": ": spaces and oracle differ in B or n",
    "lowpass": ": spaces and oracle differ in B or n",
    "svm": ": spaces and oracle differ in B or n (n = nfeat + 1)",
}
# LMI only, (streamed engine?, optim?) -> the whole text: both LDS engines use one wording, both streamed engines another
LMI_WRONG_C = {
    (False, True): "batched LMI loop: optim needs a handle made with c",
    (False, False): "batched LMI loop: feas needs a handle made without c",
    (True, True): "batched LMI streamed loop: optim needs a handle made with c",
    (True, False): "batched LMI streamed loop: feas needs a handle made without c",
}
NULL_ARGUMENT = "NULL argument"

ENTRIES = [(oracle, loop, engine) for oracle, loops in (("lmi", ("optim", "feas")), ("lowpass", ("optim", "feas")),
                                                         ("svm", ("optim",)))
           for loop in loops for engine in ENGINE_OF_KIND.values()]
assert len(ENTRIES) == 20 and len(WRONG_KIND) == 12


def entry_name(oracle, loop, engine):
    return f"ellhip_batch_{oracle}_{loop}{engine}"


def entry_id(e):
    return entry_name(*e)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what


def make_case(oracle, loop):
    if oracle == "lmi":
        problems = [lmi.family_a(s) for s in range(B)]
        return ref.lmi_feas_case(problems) if loop == "feas" else ref.lmi_case(problems)
    if oracle == "lowpass":
        return ref.lp_case(8, [lp.LOOSE, lp.family(1)], feas=loop == "feas")
    return ref.svm_case(64, 2, 1e-12, range(B))


def make_problem(gpu, case, engine, *, other_c=False):
    """the oracle handle of `case` as the engine's own constructor makes it; other_c: LMI with c where the loop wants none
    and without where it wants one"""
    streamed = engine.startswith("_streamed")
    if case.kind.startswith("lmi"):
        mat_f, mat_b, c = lmi.stack(case.problems)
        cls = gpu.BatchLmiProblem.streamed if streamed else gpu.BatchLmiProblem
        return cls(mat_f, mat_b, c if (case.kind == "lmi_optim") != other_c else None)
    if case.kind.startswith("lp"):
        cls = gpu.BatchLowpassProblem.streamed if streamed else gpu.BatchLowpassProblem
        return cls(case.n, *lp.columns(case.problems))
    cls = gpu.BatchSvmProblem.streamed if streamed else gpu.BatchSvmProblem
    return cls(np.stack([p[0] for p in case.problems]), np.stack([p[1] for p in case.problems]))


def make_batch(gpu, kind, kappa, xc):
    cls = {"lds": gpu.EllBatch, "lds_stable": gpu.EllStableBatch, "streamed": gpu.EllBatchStreamed,
           "streamed_stable": gpu.EllStableBatchStreamed}[kind]
    batch = cls.new_with_scalar(kappa, xc)
    assert batch.variant == (gpu.capi.SPACE_ELL_STABLE if kind.endswith("stable") else gpu.capi.SPACE_ELL)
    assert bool(getattr(batch, "is_streamed", False)) == kind.startswith("streamed")
    return batch


class Outputs:
    """the arrays of one raw call, filled with what a refusal must leave"""

    def __init__(self, nb, n, x_fill=-7.0):
        self.gamma = np.full(nb, 0.3)
        self.x = np.full((nb, n), x_fill)
        self.has = np.full(nb, -5, dtype=np.int32)
        self.niter = np.full(nb, -5, dtype=np.int64)
        self.status = np.full(nb, -5, dtype=np.int32)

    def untouched(self):
        return ((self.gamma == 0.3).all() and (self.x == -7.0).all() and (self.has == -5).all() and (self.niter == -5).all()
                and (self.status == -5).all())


def raw_call(lib, name, optim, batch_h, prob_h, out, tol, *, null=()):
    """the symbol itself; null: names of arguments passed as NULL"""
    ptr = lambda key: None if key in null else getattr(out, key).ctypes.data_as(C.c_void_p)
    args = ([ptr("gamma")] if optim else []) + [ROUNDS, tol, ptr("x"), ptr("has"), ptr("niter"), ptr("status")]
    return getattr(lib, name)(None if "spaces" in null else batch_h, None if "oracle" in null else prob_h, *args)


@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_raw_symbol_equals_the_mirror(gpu, entry):
    oracle, loop, engine = entry
    name, optim = entry_name(*entry), loop == "optim"
    kind = {v: k for k, v in ENGINE_OF_KIND.items()}[engine]
    case = make_case(oracle, loop)
    # the mirror, which picks the entry point from the handle
    prob, batch = make_problem(gpu, case, engine), make_batch(gpu, kind, case.kappa, case.xc)
    assert getattr(gpu, "batch_" + oracle)._loop_entry(batch, f"ellhip_batch_{oracle}_{loop}") == name
    if optim:
        x, has, niter, gamma, status = prob.optim(batch, case.gamma, ROUNDS, case.tol)
    else:
        x, has, niter, status = prob.feas(batch, ROUNDS, case.tol)
    assert niter.max() == ROUNDS, niter  # the loop ran
    # the symbol, from the same start
    prob2, batch2 = make_problem(gpu, case, engine), make_batch(gpu, kind, case.kappa, case.xc)
    out = Outputs(B, case.n, x_fill=np.nan)
    out.gamma[:] = case.gamma
    assert raw_call(gpu.capi.load(), name, optim, batch2._h, prob2._h, out, case.tol) == 0
    same(out.niter, niter, name + " niter")
    same(out.status, status, name + " status")
    same(out.has, has, name + " has")
    same(out.x, x, name + " x")
    if optim:
        same(out.gamma, gamma, name + " gamma")
    for what in ("mq", "kappa"):
        same(getattr(batch2, what), getattr(batch, what), f"{name} {what}")
    same(batch2.xc(), batch.xc(), name + " xc")


@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_refusals(gpu, entry):
    oracle, loop, engine = entry
    name, optim = entry_name(*entry), loop == "optim"
    right = {v: k for k, v in ENGINE_OF_KIND.items()}[engine]
    lib = gpu.capi.load()
    case = make_case(oracle, loop)
    prob = make_problem(gpu, case, engine)
    what = WHAT[oracle, engine]

    def refused(batch, text, p=prob, null=()):
        before = (batch.mq, batch.xc(), batch.kappa)
        out = Outputs(batch.B, batch.n)
        rc = raw_call(lib, name, optim, batch._h, p._h, out, case.tol, null=null)
        assert rc == gpu.capi.E_INVALID, (name, text, rc)
        assert lib.ellhip_last_error().decode() == text, name
        assert out.untouched(), (name, text)
        for a, b in zip(before, (batch.mq, batch.xc(), batch.kappa)):
            same(a, b, f"{name}: {text}: space")

    # each of the three other kinds of handle, of the right B and n
    for kind in KINDS:
        if kind != right:
            refused(make_batch(gpu, kind, case.kappa, case.xc), what + WRONG_KIND[engine, kind])
    # the right kind with a wrong B, with a wrong n
    refused(make_batch(gpu, right, np.full(B + 1, 10.0), np.zeros((B + 1, case.n))), what + WRONG_SHAPE[oracle])
    refused(make_batch(gpu, right, np.full(B, 10.0), np.zeros((B, case.n + 1))), what + WRONG_SHAPE[oracle])
    # a wrong kind AND a wrong B: the kind is looked at first
    other = KINDS[(KINDS.index(right) + 1) % 4]
    refused(make_batch(gpu, other, np.full(B + 1, 10.0), np.zeros((B + 1, case.n))), what + WRONG_KIND[engine, other])
    # each NULL argument (x_out may be NULL: it is optional)
    good = make_batch(gpu, right, case.kappa, case.xc)
    for arg in ("spaces", "oracle", "has", "niter", "status") + (("gamma",) if optim else ()):
        refused(good, NULL_ARGUMENT, null=(arg,))
    if oracle == "lmi":
        wrong_c = make_problem(gpu, case, engine, other_c=True)
        text = LMI_WRONG_C[engine.startswith("_streamed"), optim]
        refused(good, text, p=wrong_c)
        # ... which is looked at before the kind of the handle, and after the pointers
        refused(make_batch(gpu, other, case.kappa, case.xc), text, p=wrong_c)
        refused(good, NULL_ARGUMENT, p=wrong_c, null=("status",))


def test_the_mirror_raises_with_the_entry_points_name(gpu):
    """the EllHipError of a refused optim / feas names the entry point that refused"""
    for oracle, loop, engine in ENTRIES:
        case = make_case(oracle, loop)
        prob = make_problem(gpu, case, engine)
        kind = {v: k for k, v in ENGINE_OF_KIND.items()}[engine]
        batch = make_batch(gpu, kind, np.full(B + 1, 10.0), np.zeros((B + 1, case.n)))
        with pytest.raises(gpu.capi.EllHipError) as err:
            prob.optim(batch, math.inf, ROUNDS, case.tol) if loop == "optim" else prob.feas(batch, ROUNDS, case.tol)
        assert str(err.value) == (f"{entry_name(oracle, loop, engine)} failed with code {gpu.capi.E_INVALID}: "
                                  f"{WHAT[oracle, engine]}{WRONG_SHAPE[oracle]}")
