"""GPU: the packed group reduction in the forms that ship against the form kept as PL = 0 (group_kernels.hpp).
Kernel level (tests/cpp/group_reduce_check.hip, built with hipcc against csrc/group_kernels.hpp): k_group_reduce_p -- one clamped
strip loop over both 64-column halves, with non-temporal loads (the form for sums that come from HBM), with the heavy column blocks
first (the form for sums still in the Infinity Cache), and with all three -- gives Y and gpart word for word, from random partial
sums with a NaN in every place it must not read (3, 64, 65 and 129 strips, both segment widths, groups of 1 .. 32, every slot0 the
schedule produces, all-negative-zero inputs).
End to end: 112 parallel cuts in one queue run at n = 2048 -- on default options, and with the lower-triangle schedule and the
group stage switched on at that size (a 48-update cycle of 32 + 16, a fused pass, a second cycle) -- against the CPU oracle and,
byte for byte, between the second stream (ELLHIP_OPT_OVERLAP = 1) and the same kernels on one stream (2)."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    src = os.path.join(ROOT, "tests", "cpp", "group_reduce_check.hip")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "group_reduce_check")
    csrc = os.path.join(ROOT, "ellalgo-rs_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("group_kernels.hpp", "group_reduce_map.hpp", "ell_kernels.hpp", "ellcalc_device.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    out = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode in (0, 1), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return out


def test_reduction_equals_the_kept_form_to_the_bit(cases):
    red = [c for c in cases if c["kernel"] == "reduce"]
    assert len(red) == 15, red
    for c in red:
        print(c)
    for c in red:
        assert c["y_words_differing"] == 0 and c["gpart_words_differing"] == 0, c
        assert c["y_nans"] == 0 and c["gpart_nans"] == 0 and c["parent_nans"] == 0, c   # nothing poisoned was read
        assert c["ok"] and c["forms"] == 3, c
    plain = [c for c in red if c["mode"] == 0]
    assert {c["strips"] for c in plain} == {3, 64, 65, 129} and {c["seg"] for c in plain} == {512, 2048}
    assert {c["G"] for c in plain} == {1, 2, 15, 16, 31, 32}
    assert {(c["np"], c["slot0"]) for c in plain} == {(48, 0), (48, 16), (48, 32), (24, 8)}
    for n in (192, 4096, 4160, 8256):   # every strip count on both segment widths
        assert {c["seg"] for c in plain if c["n"] == n} == {512, 2048}, n
    assert sorted(c["mode"] for c in red if c["mode"]) == [1, 2]
    # all partial sums -0.0: the running sums start at +0.0, so the kept form gives +0.0 everywhere, and so must the clamped loop
    assert [c["y_negzeros"] for c in red if c["mode"] == 1] == [0]


N, K = 2048, 112


def _run(gpu, overlap, cuts):
    kinds, grads, b0, b1 = cuts
    e = gpu.Ell.new_with_scalar(1.0, np.zeros(N))
    e.set_option(gpu.capi.OPT_OVERLAP, overlap)
    e.profile_enable(True)
    e.queue_upload(kinds, grads, b0, b1)
    e.queue_run(0, K, fused=True)
    st, ts = e.queue_results()
    return e, st, ts, e.profile_read()


@pytest.fixture(scope="module")
def cuts_and_oracle(orc):
    from ellalgo_rs_amd import synth
    cuts = synth.parallel_cuts(N, K)
    kinds, grads, b0, b1 = cuts
    o = orc.OracleEll.new_with_scalar(1.0, np.zeros(N))
    tsq = np.empty(K)
    for i in range(K):
        assert o.update(int(kinds[i]), grads[i], b0[i], b1[i]) == 0
        tsq[i] = o.tsq
    return cuts, o, tsq


@pytest.mark.parametrize("group_stage", [False, True])
def test_queue_run_against_the_oracle_and_one_stream(gpu, cuts_and_oracle, group_stage):
    from util import TOL, rel_inf
    cuts, o, tsq = cuts_and_oracle
    capi = gpu.capi
    if group_stage:   # the schedule the benchmark times, at this size (as smoke() does)
        capi.set_default_option(capi.OPT_SYMV_MIN_N, 512)
        capi.set_default_option(capi.OPT_RESIDENT, 0)
    runs = {ov: _run(gpu, ov, cuts) for ov in (1, 2)}
    (e1, st1, ts1, p1), (e2, st2, ts2, _) = runs[1], runs[2]
    if group_stage:
        assert e1.defer_depth == 24 and e1.get_option(capi.OPT_LOOKAHEAD) == 32 and e1.get_option(capi.OPT_QUEUE_DEPTH) == 48
        # 32 + 16 | 32 + 16 | 16: the reduction of every group; the first cycle's apply pass rides on the next group's products, the
        # second cycle's stands alone (the group behind it ends the run), and the last 16 stay recorded
        assert p1["symv_reduce"][1] == 5 and p1["apply_gemv"][1] == 1 and p1["apply"][1] == 1, p1
    assert np.all(st1 == 0)
    q1 = e1.mq
    assert rel_inf(q1, o.mq) <= TOL and rel_inf(e1.xc(), np.array(o.xc)) <= TOL
    assert abs(e1.kappa - o.kappa) <= TOL * abs(o.kappa)
    assert np.max(np.abs(ts1 - tsq) / np.abs(tsq)) <= TOL
    assert st1.tobytes() == st2.tobytes() and ts1.tobytes() == ts2.tobytes()
    assert e1.xc().tobytes() == e2.xc().tobytes()
    assert np.float64(e1.kappa).tobytes() == np.float64(e2.kappa).tobytes()
    assert q1.tobytes() == e2.mq.tobytes()
