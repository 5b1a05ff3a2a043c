"""CPU: bench.py's byte models (no GPU, no engine): the passes over Q a pipelined queue run makes with the queue's
lookahead (csrc/ell_group_capi.inc.hpp queue_run_multi groups the cuts the same way) and the per-update byte counts the JSON line
carries.  Reference quantities: one update = src/ell.rs:97-137 (GEMV 8 n^2 + rank-1 16 n^2 bytes in its own data flow)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("bench_model", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_passes_over_q_with_lookahead():
    g = bench.gemv_passes
    assert g(20, 48, 16) == 2          # the driver's 20 steps: two even groups of 10
    assert g(16, 48, 16) == 1
    assert g(17, 48, 16) == 2          # 9 + 8
    assert g(48, 48, 16) == 3
    assert g(200, 48, 16) == 13        # 4 x (16 16 16) + 8
    assert g(96, 48, 16) == 6
    assert g(64, 24, 16) == 5          # depth 24 without the deeper queue: (12 12) (12 12) (16)
    assert g(24, 24, 16) == 2          # 12 + 12 rather than 16 + 8
    assert g(100, 24, 1) == 100        # one product per pass
    assert g(10, 24, 3) == 4           # vector-ALU groups: 3 3 3 1 (no even split below lookahead 4)
    # lookahead 32 (the default): groups of 17 .. 32 ride on one pass with two column tiles
    assert g(20, 48, 32) == 1          # the driver's 20 steps: one pass
    assert g(48, 48, 32) == 2          # 32 + 16
    assert g(200, 48, 32) == 9         # 4 x (32 16) + 8
    assert g(96, 48, 32) == 4
    assert g(33, 48, 32) == 2          # 32 + 1


def test_bytes_per_update():
    n2 = 16384.0 ** 2
    b, _ = bench.ell_bytes_per_update(n2, "two-pass", 1, 100, True, True)
    assert b == 24.0 * n2              # the reference's data flow
    b, _ = bench.ell_bytes_per_update(n2, "pipelined", 1, 100, True, True)
    assert b == 16.0 * n2
    b, _ = bench.ell_bytes_per_update(n2, "pipelined", 24, 48, True, True)
    assert abs(b - (4.0 + 8.0 * 2 / 48) * n2) < 1.0            # one product per pass, two apply passes
    b, text = bench.ell_bytes_per_update(n2, "pipelined", 48, 200, True, True, False, 16)
    assert abs(b - (13 * 4.0 + 5 * 8.0) / 200 * n2) < 1.0 and "lookahead 16" in text
    b, _ = bench.ell_bytes_per_update(n2, "pipelined", 24, 20, True, True, False, 16)
    assert abs(b - (2 * 4.0 + 1 * 8.0) / 20 * n2) < 1.0        # the driver's form: 0.8 n^2 per update
    b, text = bench.ell_bytes_per_update(n2 / 4, "pipelined", 48, 96, True, True, True, 16)
    assert abs(b - (6 * 4.0 + 2 * 8.0) / 96 * n2 / 4) < 1.0 and "all-reduce" in text   # symmetric shards, per GPU


def test_product_pass_roof_crosses_the_ridge_at_twenty_gradients():
    """bench.py prices the matrix-core product pass against the FP64 matrix pipe when a pass carries enough gradients to sit above
    the card's ridge (2 n^2 flop per gradient for 4 n^2 bytes: gradients / 2 flop per byte against 78.6 TFLOP/s / 8 TB/s = 9.8),
    against HBM otherwise; the numbers of profiles/r04 as the example."""
    n2 = 16384.0 ** 2
    r16 = bench.product_pass_roof(n2, 16, 0.27)
    assert r16["bound"] == "hbm" and abs(r16["flop_per_byte"] - 8.0) < 1e-12 and abs(r16["hbm_frac"] - 4 * n2 / 0.27e-3 / 8e12) < 1e-12
    r19, r20 = bench.product_pass_roof(n2, 19.6, 0.4), bench.product_pass_roof(n2, 19.7, 0.4)
    assert r19["bound"] == "hbm" and r20["bound"] == "mfma" and abs(r20["ridge"] - 9.825) < 1e-9
    r32 = bench.product_pass_roof(n2, 32, 0.445)
    assert r32["bound"] == "mfma" and abs(r32["TFLOPs"] - 2 * n2 * 32 / 0.445e-3 / 1e12) < 1e-9 and 0.48 < r32["mfma_frac"] < 0.50
    assert abs(r32["hbm_frac"] - 0.3016) < 1e-3      # the same launch against HBM: 4 n^2 bytes in 0.445 ms
    # a row shard: a quarter of the elements, a quarter of the flop and of the bytes, the same intensity
    assert bench.product_pass_roof(n2 / 4, 32, 0.2)["flop_per_byte"] == 16.0


def test_dump_sample_is_seeded_and_complete_when_small():
    import numpy as np
    a = np.arange(3000 * 1000, dtype=np.float64).reshape(3000, 1000)
    s1, s2 = bench.dump_sample(a, 4096), bench.dump_sample(a.copy(), 4096)
    assert s1.dtype == np.float64 and s1.shape == (4096,) and np.array_equal(s1, s2)   # positions depend on the size only
    assert np.all(np.diff(s1) >= 0) and np.all(np.isin(s1, a))
    small = np.arange(12, dtype=np.int32).reshape(3, 4)
    assert np.array_equal(bench.dump_sample(small, 4096), np.arange(12.0))


def test_write_outputs_float64_and_limit(tmp_path):
    import numpy as np
    import pytest
    bench.write_outputs(str(tmp_path / "d"), {"status": np.zeros(3, dtype=np.int32), "kappa": 2.5, "xc": np.ones(4)})
    got = {f: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert set(got) == {"status.npy", "kappa.npy", "xc.npy"} and all(v.dtype == np.float64 for v in got.values())
    assert got["kappa.npy"].shape == (1,) and got["kappa.npy"][0] == 2.5
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"q": np.zeros((bench.DUMP_LIMIT_BYTES // 8) + 1)})
    assert not os.path.exists(tmp_path / "big" / "q.npy")


def test_plain_and_full_options_exist():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout + r.stderr and "--dump-outputs" in r.stdout + r.stderr


@pytest.mark.parametrize("cutgen", ["parallel", "deep"])
def test_long_cut_streams_stay_valid(cutgen):
    """Offsets that follow the ellipsoid's size: many more cuts than the first few hundred, replayed on the CPU oracle, all
    succeed, every parallel cut stays parallel (b1^2 < tsq), and the predicted tsq stays close to the real one."""
    import numpy as np
    from ellalgo_rs_amd import synth
    from oracle import oracle as orc
    n, K = 512, 2500
    kinds, grads, b0, b1 = bench.cut_stream(synth, cutgen, n, K)
    _, _, r0, r1 = (synth.parallel_cuts if cutgen == "parallel" else synth.deep_cuts)(n, K)
    o = orc.OracleEll.new_with_scalar(1.0, np.zeros(n))
    ratios = []
    for i in range(K):
        assert o.update(int(kinds[i]), grads[i], float(b0[i]), None if np.isnan(b1[i]) else float(b1[i])) == 0, i
        if cutgen == "parallel":
            assert o.tsq > b1[i] ** 2, i          # o.tsq: the tsq cut i met
        raw, got = (r1[i], b1[i]) if cutgen == "parallel" else (r0[i], b0[i])
        if raw > 0:
            ratios.append(o.tsq / (got / raw) ** 2)   # real tsq / predicted tsq, every cut
    assert 0.75 < min(ratios) and max(ratios) < 1.05, (min(ratios), max(ratios))


@pytest.mark.parametrize("cutgen,n", [("parallel", 301), ("deep", 256)])
def test_cut_stream_is_synth_bit_for_bit(cutgen, n):
    """The block generator builds exactly synth's cuts (gradients, kinds, offsets before the size tracking), across the
    220-cut boundary of deep_cuts and for odd n."""
    import numpy as np
    from ellalgo_rs_amd import synth
    K = 260
    kinds, grads, b0, b1 = bench.cut_stream(synth, cutgen, n, K)
    rk, rg, r0, r1 = (synth.parallel_cuts if cutgen == "parallel" else synth.deep_cuts)(n, K)
    assert np.array_equal(kinds, rk) and np.array_equal(grads, rg)
    t0, t1 = bench.track_tsq(n, rk, r0, r1)
    assert np.array_equal(b0, t0) and np.array_equal(b1, t1, equal_nan=True)
