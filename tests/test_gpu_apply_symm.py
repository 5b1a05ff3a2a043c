"""GPU: ELLHIP_OPT_APPLY_SYMM -- the apply pass of a full set of recorded updates fused with the next group's product pass
(k_apply_symm_q) -- gives the bits of the two passes it replaces (k_apply_mfma<NP>, then k_symm_mfma_q / _q2).
Kernel level (tests/cpp/apply_symm_check.hip, built with hipcc against csrc/ell_kernels.hpp): Q, rowpart and colpart word for word,
n = 5120 / 16384, 2 .. 32 gradients, ranks 24 and 48, and a halted queue (the update lands, the products are not written).
End to end: n = 16384 handles with the option on and off on the same queued parallel cuts, with and without a cut that halts the
queue inside a 48-update cycle; the run with the option on also against the CPU oracle."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16384


def test_fused_pass_equals_apply_then_products_to_the_bit():
    src = os.path.join(ROOT, "tests", "cpp", "apply_symm_check.hip")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "apply_symm_check")
    deps = [src] + [os.path.join(ROOT, "ellalgo-rs_amd", "csrc", f) for f in ("ell_kernels.hpp", "ellcalc_device.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    cases = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(cases) == 11, (r.stdout[-2000:], r.stderr[-2000:])
    for c in cases:
        assert c["q_words_differing"] == 0 and c["rowpart_words_differing"] == 0 and c["colpart_words_differing"] == 0, c
        assert c["applied"] and c["products_as_expected"], c
        if not c["halted"]:
            assert c["queue_drawn"] >= c["tiles"], c
    assert {c["np"] for c in cases} == {24, 48} and {c["n"] for c in cases} == {5120, N}
    assert {2, 16, 17, 20, 32} <= {c["gradients"] for c in cases} and any(c["halted"] for c in cases)
    assert r.returncode == 0


def _run(gpu, on, kinds, grads, b0, b1, pieces):
    e = gpu.Ell.new_with_scalar(1.0, np.zeros(N))
    assert e.defer_depth == 24 and e.get_option(gpu.capi.OPT_LOOKAHEAD) == 32 and e.get_option(gpu.capi.OPT_QUEUE_DEPTH) == 48
    e.set_option(gpu.capi.OPT_APPLY_SYMM, on)
    assert e.get_option(gpu.capi.OPT_APPLY_SYMM) == on
    e.profile_enable(True)
    e.queue_upload(kinds, grads, b0, b1)
    for first, count in pieces:
        e.queue_run(first, count, fused=True)
    st, ts = e.queue_results()
    prof = e.profile_read()
    return e, st, ts, prof


def _same_state(a, b):
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2], equal_nan=True)
    ea, eb = a[0], b[0]
    assert np.array_equal(ea.xc(), eb.xc()) and ea.kappa == eb.kappa
    qa = ea.mq
    qb = eb.mq
    assert np.array_equal(qa, qb)
    return qa


@pytest.mark.parametrize("halt_at", [None, 71])
def test_fused_schedule_equals_separate_passes(gpu, orc, halt_at):
    """208 parallel cuts in one run: four 48-update cycles (groups of 32 and 16) and a group of 16 -- three fused passes with the
    option on, none with it off.  halt_at: a bias cut whose beta0 lies beyond tau (NoSoln) halts the queue in the second
    cycle's 32-wide group; the updates recorded before it are still owed and applied by the fused pass."""
    from ellalgo_rs_amd import synth
    from util import TOL
    k = 208
    kinds, grads, b0, b1 = synth.parallel_cuts(N, k)
    if halt_at is not None:
        b0 = b0.copy()
        b1 = b1.copy()
        b0[halt_at], b1[halt_at] = 1e6, 2e6   # beyond tau: no solution
    runs = {on: _run(gpu, on, kinds, grads, b0, b1, [(0, k)]) for on in (1, 0)}
    p1, p0 = runs[1][3], runs[0][3]
    assert p1["apply_gemv"][1] == 3 and p1["apply"][1] == 1 and p1["symv"][1] == 6, p1
    assert p0["apply_gemv"][1] == 0 and p0["apply"][1] == 4 and p0["symv"][1] == 9, p0
    st = runs[1][1]
    if halt_at is None:
        assert np.all(st == 0)
    else:
        assert np.all(st[:halt_at] == 0) and st[halt_at] == 1 and np.all(st[halt_at + 1:] == 3)
    qg = _same_state(runs[1], runs[0])
    e = runs[1][0]
    del runs
    # the oracle: the cuts that were applied (up to the halting one)
    last = k if halt_at is None else halt_at
    o = orc.OracleEll.new_with_scalar(1.0, np.zeros(N))
    for i in range(last):
        assert o.update_rowwise_mt(int(kinds[i]), grads[i], b0[i], None if np.isnan(b1[i]) else b1[i]) == 0
    ts = e.queue_results()[1]
    assert abs(e.kappa - o.kappa) <= TOL * abs(o.kappa)
    xo = np.array(o.xc)
    assert np.max(np.abs(e.xc() - xo)) <= TOL * np.max(np.abs(xo))
    qo = o.mq
    for r in range(0, N, 2048):
        assert np.max(np.abs(qg[r:r + 2048] - qo[r:r + 2048])) <= TOL * np.max(np.abs(qo[r:r + 2048])), r
    if halt_at is None:
        assert abs(ts[k - 1] - o.tsq) <= TOL * abs(o.tsq)


def test_option_is_per_handle_and_a_default(gpu):
    capi = gpu.capi
    assert capi.default_option(capi.OPT_APPLY_SYMM) == 1
    with capi.default_options({capi.OPT_APPLY_SYMM: 0}):
        e = gpu.Ell.new_with_scalar(1.0, np.zeros(1024))
        assert e.get_option(capi.OPT_APPLY_SYMM) == 0
        e.set_option(capi.OPT_APPLY_SYMM, 1)
        assert e.get_option(capi.OPT_APPLY_SYMM) == 1
    assert capi.default_option(capi.OPT_APPLY_SYMM) == 1
    with pytest.raises(Exception):
        e.set_option(capi.OPT_APPLY_SYMM, 2)
