"""The batched device-resident SVM loop against the two other ways to solve the same instances: one JSON line per shape.

  python tools/batch_svm_bench.py [--shapes 256:15:4096:shared,256:15:4096:per,96:7:163840:shared,257:31:14336:shared]
                                  [--reps 3] [--warmup 1] [--distinct 8] [--host-b 64] [--host-shapes 1] [--out F]
                                  [--space ell|stable]

Workload (tests/batch_svm_reference.py: family): only the overlapping members with shift 0.2 (s = 1, 4, 7, ...; the
separable ones end after a dozen iterations); `--distinct` of them, repeated to B.  `per`: every problem has its own
table; `shared`: the table of member 1 for every problem, the labels of problem k being member 1's with the two labels
that default_rng(k) picks exchanged.  Ell::new_with_scalar(100, 0), gamma = +inf, tol 1e-6, max_iters 4000.

Per shape:
  device   ellhip_batch_svm_optim: host clock around the whole call (state reset, gamma up, every launch, results down;
           handles are created outside the clock); --warmup calls, then --reps timed ones, each on fresh handles.
           iterations/s = rounds / t with rounds = the oracle + update rounds the instances ran (niter + 1 for an instance
           the status or the tolerance stopped).  Median, min and max are reported.
  cpu      tools/batch_svm_cpu.c: the CPU oracle's Ell update and a literal restatement of the scan in a plain C loop, one
           thread, over the distinct problems (what a one-thread sweep over all B would run at).
  host     what the engine offered before the device loop: the host computes every cut (tests/svm_reference.py: numpy
           margins, first minimum) and calls ellhip_batch_update with K = 1 per iteration (get_xc, one oracle call per
           live instance, one launch; an instance that has stopped receives a no-op cut, beta = +inf).  On the first
           --host-b instances of the first --host-shapes shapes, once.
The three forms must agree bit for bit (niter, gamma, x_best) before a rate is printed; the tool checks it.

--space stable runs the same three forms on EllStable spaces (include/ellhip_batch_stable_loops.h): the device loop on an
EllStableBatch, tools/batch_svm_cpu.c over the CPU oracle's EllStable, and the host-driven form over ellhip_batch_update
on an EllStableBatch (a stopped instance receives a cut that fails, beta = +inf).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAX_ITERS, TOL, KAPPA = 4000, 1e-6, 100.0
STABLE = False  # --space stable


def new_batch(pkg, B, n):
    return (pkg.EllStableBatch if STABLE else pkg.EllBatch).new_with_scalar(np.full(B, KAPPA), np.zeros((B, n)), device=0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rounds_of(niter):
    return int(np.sum(np.where(niter < MAX_ITERS, niter + 1, niter)))


def problems(ref, m, nfeat, distinct, shared):
    """(data, labels) of the distinct problems: data [distinct][m][nfeat], or [m][nfeat] when shared"""
    if shared:
        X, lab0 = ref.family(1, m, nfeat)
        labs = []
        for k in range(distinct):
            lab = lab0.copy()
            i, j = np.random.default_rng(k).choice(m, size=2, replace=False)
            lab[i], lab[j] = lab0[j], lab0[i]
            labs.append(lab)
        return X, np.stack(labs)
    sets = [ref.family(1 + 3 * k, m, nfeat) for k in range(distinct)]
    return np.stack([X for X, _ in sets]), np.stack([l for _, l in sets])


def tiled(data, lab, B, shared):
    reps = -(-B // lab.shape[0])
    return (data if shared else np.tile(data, (reps, 1, 1))[:B]), np.tile(lab, (reps, 1))[:B]


def device_run(pkg, data, lab):
    B, n = lab.shape[0], data.shape[-1] + 1
    prob = pkg.BatchSvmProblem(data, lab, device=0)
    batch = new_batch(pkg, B, n)
    t0 = time.perf_counter()
    x_best, has, niter, gamma, status = prob.optim(batch, math.inf, MAX_ITERS, TOL)
    return time.perf_counter() - t0, x_best, niter, gamma


def cpu_run(data, lab, shared):
    """tools/batch_svm_cpu.c over the distinct problems -> (its JSON line, niter, gamma, x_best)"""
    from oracle import oracle as O
    O.lib()  # builds oracle/libell_oracle.so when needed
    odir = os.path.join(ROOT, "oracle")
    D, m = lab.shape
    nfeat = data.shape[-1]
    full = np.ascontiguousarray(np.broadcast_to(data, (D, m, nfeat)) if shared else data)
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, f) for f in ("batch_svm_cpu", "in.bin", "out.bin"))
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-D_POSIX_C_SOURCE=199309L", "-I", odir, "-o", exe,
                               os.path.join(ROOT, "tools", "batch_svm_cpu.c"), "-L" + odir, "-lell_oracle",
                               "-Wl,-rpath," + odir, "-lm"])
        with open(fin, "wb") as f:
            f.write(struct.pack("<4qd", D, m, nfeat, MAX_ITERS, TOL) + full.tobytes() + lab.astype(np.int32).tobytes())
        line = json.loads(subprocess.run([exe, fin, fout] + (["stable"] if STABLE else []), check=True, capture_output=True,
                                         text=True).stdout)
        raw = np.fromfile(fout, dtype=np.float64).reshape(D, nfeat + 3)
    return line, raw[:, 0].copy().view(np.int64), raw[:, 1].copy(), raw[:, 2:].copy()


def host_run(pkg, svm, data, lab):
    """the form that needs no device loop: a host oracle per instance, ellhip_batch_update with K = 1 per iteration"""
    B, n = lab.shape[0], data.shape[-1] + 1
    batch = new_batch(pkg, B, n)
    gamma = np.full(B, math.inf)
    x_best = np.zeros((B, n))
    niter = np.full(B, MAX_ITERS, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    kinds = np.ones((1, B), dtype=np.int32)
    grads = np.ones((1, B, n))
    beta0 = np.full((1, B), math.inf)
    t0 = time.perf_counter()
    for it in range(MAX_ITERS):
        if not live.any():
            break
        xc = batch.xc()
        for b in np.flatnonzero(live):
            X = data if data.ndim == 2 else data[b]
            mg = svm.margins(X, lab[b], xc[b])
            idx = int(np.argmin(mg))   # the first minimum; the scan's answer when no margin is NaN
            if np.isnan(mg).any() or not mg[idx] < math.inf:
                idx = svm.argmin(mg)[0]
            val = mg[idx] if mg[idx] < math.inf else math.inf
            if val >= 1.0:
                grads[0, b], beta0[0, b], gamma[b] = 0.0, 0.0, 0.0
            else:
                y = float(lab[b, idx])
                grads[0, b, :-1], grads[0, b, -1], beta0[0, b], gamma[b] = (-y) * X[idx], -y, val, val
            x_best[b] = xc[b]
        status, tsq = batch.update(kinds, grads, beta0)
        stop = live & ((status[0] != 0) | (tsq[0] < TOL))
        niter[stop] = it
        live &= ~stop
        kinds[0, stop], grads[0, stop], beta0[0, stop] = 0, 1.0, math.inf
    return time.perf_counter() - t0, niter, gamma, x_best


def bench(pkg, ref, svm, m, nfeat, B, shared, args, with_host):
    data_d, lab_d = problems(ref, m, nfeat, args.distinct, shared)
    D = lab_d.shape[0]
    cpu, c_niter, c_gamma, c_x = cpu_run(data_d, lab_d, shared)
    data, lab = tiled(data_d, lab_d, B, shared)
    for _ in range(args.warmup):
        device_run(pkg, data, lab)
    times = []
    for _ in range(args.reps):
        dt, x_best, niter, gamma = device_run(pkg, data, lab)
        times.append(dt)
    which = np.arange(B) % D
    assert np.array_equal(niter, c_niter[which]), "device and CPU disagree (niter)"
    assert np.array_equal(bits(gamma), bits(c_gamma[which])), "device and CPU disagree (gamma)"
    assert np.array_equal(bits(x_best), bits(c_x[which])), "device and CPU disagree (x_best)"
    rounds = rounds_of(niter)
    med = statistics.median(times)
    out = {"space": "stable" if STABLE else "ell", "m": m, "nfeat": nfeat, "n": nfeat + 1, "B": B, "table": "shared" if shared else "per-problem", "distinct": D,
           "niter_min": int(niter.min()), "niter_max": int(niter.max()), "rounds": rounds,
           "table_bytes_per_iter": m * nfeat * 8,
           "device_s": {"median": med, "min": min(times), "max": max(times), "reps": args.reps},
           "device_iters_per_s": rounds / med, "device_solves_per_s": B / med,
           "cpu_s_distinct": cpu["seconds"], "cpu_iters_per_s": cpu["iters_per_s"],
           "device_over_cpu": rounds / med / cpu["iters_per_s"]}
    if with_host:
        hb = min(B, args.host_b)
        dt, niter_h, gamma_h, x_h = host_run(pkg, svm, data if shared else data[:hb], lab[:hb])
        assert np.array_equal(niter_h, niter[:hb]), "device and host-driven form disagree (niter)"
        assert np.array_equal(bits(gamma_h), bits(gamma[:hb])), "device and host-driven form disagree (gamma)"
        assert np.array_equal(bits(x_h), bits(x_best[:hb])), "device and host-driven form disagree (x_best)"
        host_rate = rounds_of(niter_h) / dt
        out.update(host_B=hb, host_s=dt, host_iters_per_s=host_rate, device_over_host=rounds / med / host_rate)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256:15:4096:shared,256:15:4096:per,96:7:163840:shared,257:31:14336:shared")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--host-b", type=int, default=64)
    ap.add_argument("--host-shapes", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--space", choices=("ell", "stable"), default="ell")
    args = ap.parse_args()
    global STABLE
    STABLE = args.space == "stable"
    import ellalgo_rs_amd as pkg
    import batch_svm_reference as ref
    import svm_reference as svm
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched svm loop has no CPU path")
    for k, shape in enumerate(args.shapes.split(",")):
        m, nfeat, B, kind = shape.split(":")
        res = bench(pkg, ref, svm, int(m), int(nfeat), int(B), kind == "shared", args, k < args.host_shapes)
        line = json.dumps({"bench": "batch_svm", **res})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
