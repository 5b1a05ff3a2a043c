"""GPU: every FP64 matrix-core pass, by itself, against an extended-precision reference of the same operation, ELEMENT BY ELEMENT
(tests/cpp/matrix_core_reference_check.hip, built with hipcc against csrc/ell_kernels.hpp and group_kernels.hpp; the reference and
the derived bounds are tests/cpp/ext_reference.hpp, pinned on the CPU by tests/test_ext_reference_cpu.py):

    products  |yhat[r] - y[r]| <= (n + nstrips + nsegs + 8) 2^-53 S[r]      k_symm_mfma, k_symm_mfma_q, k_symm_mfma_q2 (+ packed)
    apply     |xhat - X|       <= 2 NP 2^-53 M                              k_apply_mfma<24 | 48>, k_apply_symm_q
    bit for bit against the two-rounding sequence of its header             k_apply_lower<8 | 16>

on graded inputs (every element at its own scale, 2^-60 .. 2^60) whose strict upper triangle, padding, unused operand slots and
guard bands hold NaN.  The other kernel-level checks (symm_queue_check, apply_symm_check, packed_operands_check) compare kernel with
kernel, bit for bit: they rest on this anchor.  One subprocess per group, no retry."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL = [(64, 512), (128, 512), (320, 512), (320, 2048), (576, 512), (1088, 512), (1088, 2048)]   # (n, SEG), unsharded
SHARDS = [(576, 64, 256), (576, 320, 256), (1088, 512, 576)]                                     # (n, row0, nrows), SEG 512
LV16, LV32 = (1, 2, 15, 16), (17, 31, 32)


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "cpp", "matrix_core_reference_check.hip")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "matrix_core_reference_check")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "ext_reference.hpp")]
    deps += [os.path.join(ROOT, "ellalgo-rs_amd", "csrc", f) for f in ("ell_kernels.hpp", "group_kernels.hpp", "ellcalc_device.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    return exe


def _run(exe, group, expected):
    r = subprocess.run([exe, group], capture_output=True, text=True, timeout=600)
    cases = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(cases) == expected, (len(cases), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    for c in cases:
        print(json.dumps(c))
    return r, cases


def _key(c):
    return (c["kernel"], c["pk"], c["n"], c["seg"], c["lv"], (c["row0"], c["nrows"]), c["halted"])


def _product_keys():
    want = set()
    shapes = [(n, seg, 0, n) for n, seg in FULL] + [(n, 512, r0, nr) for n, r0, nr in SHARDS]
    for n, seg, r0, nr in shapes:
        for lv in LV16:
            want.add(("k_symm_mfma", False, n, seg, lv, (r0, nr), False))
            want |= {("k_symm_mfma_q", pk, n, seg, lv, (r0, nr), False) for pk in (False, True)}
        for lv in LV32:
            want |= {("k_symm_mfma_q2", pk, n, seg, lv, (r0, nr), False) for pk in (False, True)}
    want |= {("k_symm_mfma_q2", pk, 2112, 2048, 17, (0, 2112), False) for pk in (False, True)}
    return want


def test_product_passes_hold_the_elementwise_bound(exe):
    want = _product_keys()
    r, cases = _run(exe, "products", len(want) + 5)
    got = {_key(c) for c in cases}
    assert want <= got, sorted(want - got)
    halted = {(c["kernel"], c["pk"]) for c in cases if c["halted"]}
    assert halted == {("k_symm_mfma", False)} | {(k, pk) for k in ("k_symm_mfma_q", "k_symm_mfma_q2") for pk in (False, True)}
    for c in cases:
        assert c["ratio_partials"] <= 1.0 and c["ratio_y"] <= 1.0 and c["first_bad"] == -1, c
        assert c["q_kept"] and c["untouched_kept"] and c["guards_kept"] and c["stray_words"] == 0 and c["queue_ok"], c
        if not c["halted"]:
            assert c["ratio_partials"] > 0.0, c
            # the project's own reduction ran too (the packed one is for unsharded handles)
            assert c["reduced"] == (not c["pk"] or c["row0"] == 0 and c["nrows"] == c["n"]), c
            assert not c["reduced"] or c["ratio_y"] > 0.0, c
    assert r.returncode == 0, r.stderr[-2000:]


def test_apply_passes_hold_the_elementwise_bound(exe):
    ns = [n for n, _ in FULL if _ == 512] + [2112, 1000]
    want = {(k, np_, n, 0, n) for n in ns for k, np_ in (("k_apply_mfma", 24), ("k_apply_mfma", 48), ("k_apply_lower", 8),
                                                         ("k_apply_lower", 16))}
    want |= {("k_apply_mfma", np_, n, r0, nr) for n, r0, nr in SHARDS for np_ in (24, 48)}
    r, cases = _run(exe, "apply", len(want))
    assert {(c["kernel"], c["np"], c["n"], c["row0"], c["nrows"]) for c in cases} == want
    for c in cases:
        assert 0.0 < c["ratio_q"] <= 1.0 and c["first_bad"] == -1, c
        assert c["right_of_strip_changed"] == 0 and c["inputs_kept"] and c["guards_kept"], c
        if c["kernel"] == "k_apply_lower":   # "the reference's sequence of roundings", to the bit
            assert c["differ_from_two_roundings"] == 0, c
        else:                                # one rounding per update: not the two-rounding form (reported)
            assert c["differ_from_two_roundings"] > 0, c
    assert r.returncode == 0, r.stderr[-2000:]


def test_fused_pass_holds_both_elementwise_bounds(exe):
    want = {(pk, n, seg, lv) for n, seg in FULL for lv in LV16 + LV32 for pk in (False, True)}
    want |= {(pk, 2112, 2048, 17) for pk in (False, True)}
    r, cases = _run(exe, "fused", len(want) + 2)
    live = [c for c in cases if not c["halted"]]
    assert {(c["pk"], c["n"], c["seg"], c["lv"]) for c in live} == want
    assert {(c["np"], c["lv"] > 16, c["pk"]) for c in live} == {(np_, w, pk) for np_ in (24, 48) for w in (False, True) for pk in (False, True)}
    assert sorted((c["pk"], c["lv"] > 16) for c in cases if c["halted"]) == [(False, False), (True, True)]
    for c in cases:
        assert 0.0 < c["ratio_q"] <= 1.0 and c["first_bad"] == -1, c          # halted or not, the update lands
        assert c["ratio_partials"] <= 1.0 and c["ratio_y"] <= 1.0, c
        assert c["untouched_kept"] and c["guards_kept"] and c["inputs_kept"] and c["stray_words"] == 0 and c["queue_ok"], c
        assert c["right_of_strip_changed"] == 0, c
        if not c["halted"]:
            assert c["ratio_partials"] > 0.0 and c["reduced"] and c["ratio_y"] > 0.0, c
    assert r.returncode == 0, r.stderr[-2000:]
