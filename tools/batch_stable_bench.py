#!/usr/bin/env python3
"""Throughput of the batched engine's EllStable variant (include/ellhip_batch.h).

For each n: B ellipsoids sized to fill the card (several rounds of workgroups on every CU), K central cuts each per launch
(they always succeed), every input resident in HBM (ellhip_batch_update_dev), started from a random factor.  Value =
ellipsoid updates/s summed over the batch.  Next to it, the one-thread CPU rate of the oracle's EllStable update in a
plain C loop (tools/batch_stable_cpu.c).  One JSON line per n.

    python3 tools/batch_stable_bench.py [--sizes 2,3,16,64,128] [--steps 20] [--warmup 3] [--cpu-seconds 2] [--out F]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 8
CUS = 256
# ellipsoids per launch: n -> B (four or more rounds of the resident workgroups of every CU)
POP = {2: 524288, 3: 524288, 16: 65536, 64: 4096, 128: 1024}
HBM_PEAK_GBS = 8000.0


def random_factors(B, n, rng):
    m = rng.standard_normal((n, n)) * (0.1 / np.sqrt(n))
    m[np.arange(n), np.arange(n)] = 0.5 + rng.random(n)
    return np.broadcast_to(m, (B, n, n))


def gpu_rate(pkg, n, B, steps, warmup):
    hip = C.CDLL(sorted(pkg.capi.mapped_runtimes()["libamdhip64"])[0])  # the runtime the engine is bound to
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    rng = np.random.default_rng(0x5EED + n)
    grads = rng.standard_normal((K, B, n))
    grads /= np.linalg.norm(grads, axis=2, keepdims=True)
    host = [np.full((K, B), 1, dtype=np.int32), grads, np.zeros((K, B)), np.zeros((K, B), dtype=np.int32),
            np.zeros((K, B))]
    status = np.full((K, B), -1, dtype=np.int32)
    batch = pkg.EllStableBatch.new_with_matrix(1.0, random_factors(B, n, rng), np.zeros((B, n)))
    ptrs = []
    try:
        for x in host + [status]:
            p = C.c_void_p()
            if hip.hipMalloc(C.byref(p), x.nbytes) != 0:
                raise RuntimeError("hipMalloc failed")
            ptrs.append(p)
        for p, x in zip(ptrs, host + [status]):
            if hip.hipMemcpy(p, x.ctypes.data, x.nbytes, 1) != 0:
                raise RuntimeError("hipMemcpy failed")

        def launch():
            batch.update_dev(K, *ptrs[:5], ptrs[5], None)

        for _ in range(warmup):
            launch()
        batch.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            launch()
        batch.synchronize()
        elapsed = time.perf_counter() - t0
        if hip.hipMemcpy(status.ctypes.data, ptrs[5], status.nbytes, 2) != 0:
            raise RuntimeError("hipMemcpy failed")
    finally:
        for p in ptrs:
            hip.hipFree(p)
    if not (status == 0).all():
        raise RuntimeError(f"n={n}: a central cut did not succeed")
    tsq = batch.tsq()
    if not np.isfinite(tsq).all():
        raise RuntimeError(f"n={n}: non-finite tsq")
    return elapsed, steps


def cpu_rate(n, seconds):
    from oracle import oracle as O
    O.lib()  # builds oracle/libell_oracle.so when needed
    odir = os.path.join(ROOT, "oracle")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "batch_stable_cpu")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-D_POSIX_C_SOURCE=199309L", "-I", odir,
                               "-o", exe, os.path.join(ROOT, "tools", "batch_stable_cpu.c"), "-L" + odir, "-lell_oracle",
                               "-Wl,-rpath," + odir, "-lm"])
        B = max(1, min(4096, (1 << 22) // (n * n)))  # a working set of at most 32 MiB
        out = subprocess.run([exe, str(n), str(B), str(K), str(seconds)], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="2,3,16,64,128")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-seconds", type=float, default=2.0, help="0: no CPU column")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import ellalgo_rs_amd as pkg
    pkg.capi.load()
    for n in (int(s) for s in args.sizes.split(",")):
        B = POP.get(n, 65536)
        elapsed, steps = gpu_rate(pkg, n, B, args.steps, args.warmup)
        ms = elapsed / steps * 1e3
        alg = B * (16.0 * n * n + K * (8.0 * n + 24.0) + 16.0 * n + 16.0)  # per launch: buffer in + out, cuts, xc, scalars
        rec = {"workload": f"ellstable-batch-n{n}", "n": n, "ellipsoids": B, "cuts_per_launch": K, "launches": steps,
               "ms_per_launch": ms, "updates_per_s": steps * K * B / elapsed,
               "byte_model_gbs": alg / (ms * 1e-3) / 1e9, "byte_model_frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
               "cuts": "central, random unit gradients", "start": "random unit-upper factor, junk in the scratch triangle",
               "timing": "wall clock over the launches, inputs resident (ellhip_batch_update_dev)"}
        if args.cpu_seconds > 0:
            c = cpu_rate(n, args.cpu_seconds)
            rec["cpu_1thread_updates_per_s"] = c["updates_per_s"]
            rec["cpu_sample"] = (f"{c['updates']} updates, {c['B']} spaces x {c['K']} central cuts per round, oracle "
                                 f"orc_ellstable_update in a C loop, 1 thread, {c['seconds']:.1f} s")
            rec["speedup_vs_cpu_1thread"] = rec["updates_per_s"] / c["updates_per_s"]
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
