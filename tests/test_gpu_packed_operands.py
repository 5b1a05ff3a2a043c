"""GPU: ELLHIP_OPT_PACKED_OPERANDS -- the matrix-core passes fetch the group's gradients and the recorded vectors from copies in
MFMA operand order and store the column sums of two cuts side by side (16 bytes per lane and instruction) -- gives the bits of
the unpacked kernels.
Kernel level (tests/cpp/packed_operands_check.hip, built with hipcc against csrc/group_kernels.hpp): Q after the fused pass,
rowpart, colpart with the pairing undone, and Y / gpart of the two reduce forms word for word; n = 320 / 1088 (and 4160 for the
reduce kernels' unrolled strip loops), segments of 512 and 2048 columns, 2 .. 32 gradients, ranks 24 and 48, 0 / 16 / 48 recorded
slots, halted queues.  Row shards keep the unpacked kernels, so there is no shard case.
End to end: one n = 5120 handle per setting on the same 160 queued parallel cuts (three 48-update cycles, two fused passes), with
and without a cut that halts the queue inside the second cycle; the run with the option on also against the CPU oracle."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5120
K = 160
LVS = {2, 15, 16, 17, 20, 31, 32}


def test_packed_kernels_equal_unpacked_to_the_bit():
    src = os.path.join(ROOT, "tests", "cpp", "packed_operands_check.hip")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "packed_operands_check")
    deps = [src] + [os.path.join(ROOT, "ellalgo-rs_amd", "csrc", f) for f in ("ell_kernels.hpp", "group_kernels.hpp", "ellcalc_device.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    cases = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(cases) == 22, (r.stdout[-2000:], r.stderr[-2000:])
    for c in cases:
        print(c)
    for c in cases:
        assert c["q_words_differing"] == 0 and c["rowpart_words_differing"] == 0 and c["colpart_words_differing"] == 0, c
        assert c["y_words_differing"] == 0 and c["gpart_words_differing"] == 0, c
        assert c["applied"] and c["products_as_expected"] and c["reduced_as_expected"], c
        if not c["halted"]:
            assert c["queue_drawn"] >= c["tiles"], c
    for n in (320, 1088):
        assert {c["gradients"] for c in cases if c["n"] == n and c["seg"] == 512 and not c["halted"]} == LVS
        assert {c["seg"] for c in cases if c["n"] == n} == {512, 2048}
        assert {c["np"] for c in cases if c["n"] == n} == {24, 48}
    assert any(c["halted"] for c in cases) and any(c["strips"] > 64 for c in cases)
    assert r.returncode == 0


def _run(gpu, on, kinds, grads, b0, b1):
    e = gpu.Ell.new_with_scalar(1.0, np.zeros(N))
    assert e.defer_depth == 24 and e.get_option(gpu.capi.OPT_LOOKAHEAD) == 32 and e.get_option(gpu.capi.OPT_QUEUE_DEPTH) == 48
    e.set_option(gpu.capi.OPT_PACKED_OPERANDS, on)
    assert e.get_option(gpu.capi.OPT_PACKED_OPERANDS) == on
    e.profile_enable(True)
    e.queue_upload(kinds, grads, b0, b1)
    e.queue_run(0, K, fused=True)
    st, ts = e.queue_results()
    prof = e.profile_read()
    return e, st, ts, prof


@pytest.fixture(scope="module")
def cuts():
    from ellalgo_rs_amd import synth
    return synth.parallel_cuts(N, K)


@pytest.mark.parametrize("halt_at", [None, 71])
def test_packed_run_equals_unpacked_run(gpu, orc, cuts, halt_at):
    """160 parallel cuts in one run: three 48-update cycles (groups of 32 and 16) and a group of 16 -- two fused passes.
    halt_at: a cut whose beta0 lies beyond tau (NoSoln) halts the queue in the second cycle's 32-wide group; the updates recorded
    before it are still owed and applied."""
    from util import TOL
    kinds, grads, b0, b1 = cuts
    if halt_at is not None:
        b0 = b0.copy()
        b1 = b1.copy()
        b0[halt_at], b1[halt_at] = 1e6, 2e6   # beyond tau: no solution
    runs = {on: _run(gpu, on, kinds, grads, b0, b1) for on in (1, 0)}
    (e1, st1, ts1, p1), (e0, st0, ts0, p0) = runs[1], runs[0]
    assert p1["apply_gemv"][1] == 2, p1
    for cls in p1:
        assert p1[cls][1] == p0[cls][1], (cls, p1, p0)   # launch counts, class by class
    assert np.array_equal(st1, st0) and np.array_equal(ts1, ts0, equal_nan=True)
    if halt_at is None:
        assert np.all(st1 == 0)
    else:
        assert np.all(st1[:halt_at] == 0) and st1[halt_at] == 1 and np.all(st1[halt_at + 1:] == 3)
    assert np.array_equal(e1.xc(), e0.xc()) and e1.kappa == e0.kappa
    q1 = e1.mq
    assert np.array_equal(q1, e0.mq)
    del runs, e0
    # the oracle: the cuts that were applied (up to the halting one)
    last = K if halt_at is None else halt_at
    o = orc.OracleEll.new_with_scalar(1.0, np.zeros(N))
    for i in range(last):
        assert o.update_rowwise_mt(int(kinds[i]), grads[i], b0[i], None if np.isnan(b1[i]) else b1[i]) == 0
    assert abs(e1.kappa - o.kappa) <= TOL * abs(o.kappa)
    xo = np.array(o.xc)
    assert np.max(np.abs(e1.xc() - xo)) <= TOL * np.max(np.abs(xo))
    qo = o.mq
    for r in range(0, N, 1024):
        assert np.max(np.abs(q1[r:r + 1024] - qo[r:r + 1024])) <= TOL * np.max(np.abs(qo[r:r + 1024])), r
    if halt_at is None:
        assert abs(ts1[K - 1] - o.tsq) <= TOL * abs(o.tsq)


def test_option_is_per_handle_and_a_default(gpu):
    capi = gpu.capi
    try:
        assert capi.default_option(capi.OPT_PACKED_OPERANDS) == 1
        with capi.default_options({capi.OPT_PACKED_OPERANDS: 0}):
            e = gpu.Ell.new_with_scalar(1.0, np.zeros(1024))
            assert e.get_option(capi.OPT_PACKED_OPERANDS) == 0
            e.set_option(capi.OPT_PACKED_OPERANDS, 1)
            assert e.get_option(capi.OPT_PACKED_OPERANDS) == 1
        assert capi.default_option(capi.OPT_PACKED_OPERANDS) == 1
        with pytest.raises(Exception):
            e.set_option(capi.OPT_PACKED_OPERANDS, 2)
        with pytest.raises(Exception):
            capi.set_default_option(capi.OPT_PACKED_OPERANDS, 2)
        assert e.get_option(capi.OPT_PACKED_OPERANDS) == 1
    finally:
        capi.set_default_option(capi.OPT_PACKED_OPERANDS, 1)   # (the suite's factory-default list predates the option)
