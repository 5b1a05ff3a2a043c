"""SvmOracle on the device: one JSON line per table size.

  python tools/svm_bench.py [--sizes 1048576:511,65536:255] [--calls 50] [--iters 200] [--cpu]

Per size (m samples x nfeat features, search space n = nfeat + 1 on an Ell at its default depth):
  oracle_ms          one ellhip_svm_assess_optim (x up, the scan, the cut down), host clock around calls that each
                     end in a stream synchronise; median of --calls
  oracle_bytes       the byte model of one scan: m * nfeat * 8 (the table, read once) + 4 m (labels)
  oracle_tbps        oracle_bytes / oracle_ms, and its share of the 8 TB/s HBM peak (a whole-call rate: it includes the
                     copies of x and of the gradient and both launches; kernel times come from a rocprofv3 run)
  loop_device_it_s   iterations / s of ellhip_svm_optim (the device-resident loop), --iters iterations, tol = 0
  loop_host_it_s     iterations / s of the host-driven loop: assess_optim + ellhip_update (update_central_cut)
  loop_bytes_*       the byte model per iteration: the scan plus the update's own bytes at its schedule
                     (depth 1: 16 n^2 for the device loop, whose shrink carries the next GEMV; 24 n^2 host-driven)
  cpu_ms             (--cpu) one call of the numpy restatement of the reference (tests/svm_reference.py), on this
                     host's CPU: the left fold vectorised over samples plus the argmin loop; a CPU time, not the GPU's

Data: a seeded uniform table with labels independent of it (not separable, so a loop with tol = 0 runs all --iters).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TBPS = 8.0


def make_table(m: int, nfeat: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    data = np.empty((m, nfeat), dtype=np.float64)
    rows = max(1, (64 << 20) // (8 * nfeat))
    for r0 in range(0, m, rows):
        data[r0:r0 + rows] = rng.random((min(rows, m - r0), nfeat)) - 0.5
    labels = np.where(rng.random(m) < 0.5, -1, 1).astype(np.int32)
    return data, labels


def host_loop(o, space, gamma, iters):
    for _ in range(iters):
        cut, _, gamma = o.assess_optim(space.xc(), gamma)
        if int(space.update_central_cut(cut)) != 0:
            break
    return gamma


def bench_size(pkg, m: int, nfeat: int, calls: int, iters: int, cpu: bool) -> dict:
    data, labels = make_table(m, nfeat)
    t0 = time.perf_counter()
    o = pkg.SvmOracle(data, labels, device=0)
    create_s = time.perf_counter() - t0
    n = nfeat + 1
    rng = np.random.default_rng(1)
    x = rng.standard_normal(n) * 0.01
    for _ in range(3):  # warm-up: code objects, first touch
        o.assess_optim(x, 0.0)
    ts = []
    for _ in range(calls):
        t = time.perf_counter()
        o.assess_optim(x, 0.0)
        ts.append(time.perf_counter() - t)
    oracle_s = statistics.median(ts)
    scan_bytes = m * nfeat * 8 + 4 * m
    # loops: the device-resident one and the host-driven one, same space type and depth, same number of iterations
    sp = pkg.Ell.new_with_scalar(10.0, np.zeros(n), device=0)
    depth = sp.defer_depth
    o.cutting_plane_optim(sp, 0.0, 3, 0.0)  # warm-up
    sp = pkg.Ell.new_with_scalar(10.0, np.zeros(n), device=0)
    t = time.perf_counter()
    _, niter_d, _ = o.cutting_plane_optim(sp, 0.0, iters, 0.0)
    dev_s = time.perf_counter() - t
    sh = pkg.Ell.new_with_scalar(10.0, np.zeros(n), device=0)
    host_loop(o, sh, 0.0, 3)
    sh = pkg.Ell.new_with_scalar(10.0, np.zeros(n), device=0)
    t = time.perf_counter()
    host_loop(o, sh, 0.0, iters)
    host_s = time.perf_counter() - t
    upd_dev = (16 if depth == 1 else 8) * n * n
    upd_host = (24 if depth == 1 else 8) * n * n
    out = dict(tool="svm_bench", m=m, nfeat=nfeat, n=n, table_bytes=int(nfeat * (-(-m // 8) * 8) * 8),
               beyond_infinity_cache=bool(nfeat * m * 8 > (256 << 20)), create_s=round(create_s, 3),
               oracle_calls=calls, oracle_ms=round(oracle_s * 1e3, 4), oracle_ms_min=round(min(ts) * 1e3, 4),
               oracle_bytes=scan_bytes, oracle_tbps=round(scan_bytes / oracle_s / 1e12, 3),
               oracle_share_of_peak=round(scan_bytes / oracle_s / 1e12 / PEAK_TBPS, 3),
               loop_depth=depth, loop_iters=iters, loop_device_niter=niter_d,
               loop_device_it_s=round(niter_d / dev_s, 2), loop_host_it_s=round(iters / host_s, 2),
               loop_bytes_device=scan_bytes + upd_dev, loop_bytes_host=scan_bytes + upd_host,
               loop_device_tbps=round(niter_d * (scan_bytes + upd_dev) / dev_s / 1e12, 3),
               loop_host_tbps=round(iters * (scan_bytes + upd_host) / host_s / 1e12, 3))
    if cpu:
        import svm_reference as ref
        t = time.perf_counter()
        ref.argmin(ref.margins(data, labels, x))
        out["cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        out["cpu_what"] = "numpy restatement of the reference, one call, one host thread"
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1048576:511,65536:255", help="comma-separated m:nfeat")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement once per size")
    args = ap.parse_args()
    import ellalgo_rs_amd as pkg
    if pkg.capi.load().ellhip_device_count() <= 0:
        print("svm_bench: no HIP device (the oracle has no CPU path)", file=sys.stderr)
        return 2
    for spec in args.sizes.split(","):
        m, nfeat = (int(v) for v in spec.split(":"))
        print(json.dumps(bench_size(pkg, m, nfeat, args.calls, args.iters, args.cpu)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
