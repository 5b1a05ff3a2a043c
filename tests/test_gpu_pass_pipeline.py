"""GPU: the rotated block loops of the 32-wide product pass (k_symm_mfma_q2) and of the fused apply + product pass
(k_apply_symm_q) -- next block loaded behind the row products, the strip's A operands read in pairs, the update accumulators
taken one after the other -- give the bits of the loops they replace.
Kernel level (tests/cpp/pass_pipeline_check.hip, built with hipcc against csrc/ell_kernels.hpp): the shipped loops against the
old ones (template argument PL = 0) on Q, rowpart and colpart word for word, NaN in the upper triangle of Q and in every slot of
the partial sums beforehand; n = 64 / 128 / 576 / 1088 in segments of 512 columns, 2112 / 4160 in segments of 2048, 1 .. 32
gradients, ranks 24 and 48, queue halted and not, packed and unpacked operands.
End to end: queue runs of 56 and 112 cuts at n = 5120 against the CPU oracle (the second one holds a fused pass)."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = {512: {64, 128, 576, 1088}, 2048: {2112, 4160}}
LVS = {1, 16, 17, 31, 32}


def test_rotated_loops_equal_old_loops_to_the_bit():
    src = os.path.join(ROOT, "tests", "cpp", "pass_pipeline_check.hip")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pass_pipeline_check")
    deps = [src] + [os.path.join(ROOT, "ellalgo-rs_amd", "csrc", f) for f in ("ell_kernels.hpp", "ellcalc_device.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    # one process, one time limit: a fault ends it and nothing else is started on the card by this test
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    cases = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    want = {(n, seg, lv, np_, halted, packed) for seg, ns in NS.items() for n in ns for lv in LVS for np_ in (24, 48)
            for halted in (False, True) for packed in (False, True)}
    got = {(c["n"], c["seg"], c["gradients"], c["np"], c["halted"], c["packed"]) for c in cases}
    assert got == want and len(cases) == len(want) == 240, (len(cases), sorted(want - got)[:5], r.stderr[-2000:])
    for c in cases:
        assert c["q_words_differing"] == 0 and c["rowpart_words_differing"] == 0 and c["colpart_words_differing"] == 0, c
        assert c["applied"] and c["slots_written_as_expected"], c
        assert c["queue_drawn"] >= c["tiles"], c
    assert r.returncode == 0


@pytest.mark.parametrize("k, fused", [(56, 0), (112, 1)])
def test_queue_run_against_the_oracle(gpu, orc, k, fused):
    """56 cuts: groups of 32 and 16, then the run's last 8 cuts behind a separate apply pass -- the rotated 32-wide product pass
    opens the run.  112 cuts: the first 48 recorded updates are applied by the fused pass (rank 48, rotated, segments of 512
    columns) under the products of the second cycle's 32 cuts."""
    from ellalgo_rs_amd import synth
    from util import TOL
    n = 5120
    kinds, grads, b0, b1 = synth.parallel_cuts(n, k)
    e = gpu.Ell.new_with_scalar(1.0, np.zeros(n))
    assert e.defer_depth == 24 and e.get_option(gpu.capi.OPT_LOOKAHEAD) == 32 and e.get_option(gpu.capi.OPT_QUEUE_DEPTH) == 48
    assert e.get_option(gpu.capi.OPT_APPLY_SYMM) == 1 and e.get_option(gpu.capi.OPT_PACKED_OPERANDS) == 1
    e.profile_enable(True)
    e.queue_upload(kinds, grads, b0, b1)
    e.queue_run(0, k, fused=True)
    st, ts = e.queue_results()
    prof = e.profile_read()
    assert prof["apply_gemv"][1] == fused, prof
    assert np.all(st == 0)
    o = orc.OracleEll.new_with_scalar(1.0, np.zeros(n))
    for i in range(k):
        assert o.update_rowwise_mt(int(kinds[i]), grads[i], b0[i], None if np.isnan(b1[i]) else b1[i]) == 0
    assert abs(e.kappa - o.kappa) <= TOL * abs(o.kappa)
    xo = np.array(o.xc)
    assert np.max(np.abs(e.xc() - xo)) <= TOL * np.max(np.abs(xo))
    qg, qo = e.mq, o.mq
    for r in range(0, n, 1024):
        assert np.max(np.abs(qg[r:r + 1024] - qo[r:r + 1024])) <= TOL * np.max(np.abs(qo[r:r + 1024])), r
    assert abs(ts[k - 1] - o.tsq) <= TOL * abs(o.tsq)
