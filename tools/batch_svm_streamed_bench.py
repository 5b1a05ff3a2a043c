"""The batched device-resident SVM loop on streamed batch handles (include/ellhip_batch_svm_streamed.h)
beside three baselines: one JSON line per shape, then one line per n with the oracle's share of a round.

  python tools/batch_svm_streamed_bench.py [--space ell|stable] [--shared] [--nfeat 128,255,511,1023] [--m-over-n 0.5,2,8]
                                           [--batches 1536,1536,768,256] [--iters 1500,600,200,60] [--distinct 6]
                                           [--reps 3] [--warmup 1] [--seconds 0.5] [--table-cap-gib 4] [--out FILE]

A shape is (nfeat, m, B): n = nfeat + 1 = 129, 256, 512 and 1024 by default, m = n / 2, 2 n and 8 n, and B per n as
tools/batch_lowpass_streamed_bench.py chooses it (--space stable: 1536, 512, 512, 512).  Workload
(tests/batch_svm_reference.py: family): the overlapping members with shift 0.2 (s = 1, 4, 7, ...; they never end early),
--distinct of them repeated to B, every problem with its own table, or with --shared the table of member 1 and labels that
differ in two places per problem (tools/batch_svm_bench.py: problems).  Without --shared B is lowered until the tables fit
--table-cap-gib.  new_with_scalar(100, 0), gamma = +inf, tol 1e-12, cut off at the n's --iters (every problem runs every
round; the one-thread CPU column, at a few hundred rounds/s at n = 1024, is what keeps the counts this low).

  device   ellhip_batch_svm_optim_streamed / _streamed_stable: host clock around the whole call (state reset, gamma up, the
           launches, results down) on fresh spaces; the oracle handle is made once per shape.  --warmup calls, then --reps.
  (a) cpu  tools/batch_svm_cpu.c: the CPU oracle's update and a literal restatement of the scan in a plain C loop, one
           thread, over the distinct problems.
  (b) host the host-driven form on the same kind of streamed handle: per iteration ellhip_batch_get_xc, one wide
           ellhip_batch_svm_assess_optim (the same device oracle, one workgroup per problem) and one ellhip_batch_update with
           K = 1, for all B problems.  Once per shape, after three warm-up iterations.
  (c) plain the streamed engine's own update rate at the same (n, B), cut inputs resident in HBM, K = 1 and K = 8 cuts per
           launch (tools/batch_streamed_bench.py: DevArrays, window), in the same process.
Rates are rounds per second (oracle + update), all problems together.  Before a rate is printed the device result must equal
(a) and (b) bit for bit: niter, gamma, x_best.

Model printed beside the measurements, per problem and round: 16 n^2 bytes of matrix (Ell; the product of round k + 1 rides
on the sweep of round k) or 24 n^2 (EllStable), 8 nfeat m bytes of table and 4 m of labels; model_GB_per_s is the device rate
under it.  fold_chain: the ceil(m / n) * nfeat dependent multiply-add pairs of one thread's scan.  The closing line per n fits
seconds per round = t0 + c m over the n's shapes and gives c m / (t0 + c m), the share of a round that grows with m."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TOL, KAPPA = 1e-12, 100.0
STABLE = False  # --space stable


def batch_class(pkg):
    return pkg.EllStableBatchStreamed if STABLE else pkg.EllBatchStreamed


def new_spaces(pkg, B, n, kappa=KAPPA):
    return batch_class(pkg).new_with_scalar(np.full(B, kappa), np.zeros((B, n)), device=0)


def device_run(pkg, prob, max_iters):
    batch = new_spaces(pkg, prob.B, prob.n)
    batch.synchronize()
    t0 = time.perf_counter()
    x_best, has, niter, gamma, status = prob.optim(batch, math.inf, max_iters, TOL)
    return time.perf_counter() - t0, x_best, niter, gamma


def host_run(pkg, prob, max_iters):
    """(b): the oracle on the device, one call per iteration, and ellhip_batch_update with K = 1; a problem that has stopped
    receives a cut that fails (beta = +inf)"""
    B, n = prob.B, prob.n
    batch = new_spaces(pkg, B, n)
    gamma = np.full(B, math.inf)
    x_best = np.zeros((B, n))
    niter = np.full(B, max_iters, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    kinds = np.ones((1, B), dtype=np.int32)
    beta0 = np.zeros((1, B))
    t0 = time.perf_counter()
    for it in range(max_iters):
        if not live.any():
            break
        xc = batch.xc()
        grad, beta, g = prob.assess_optim(xc)
        gamma[live] = g[live]
        x_best[live] = xc[live]
        grads = grad[None]
        beta0[0] = beta
        grads[0, ~live], beta0[0, ~live], kinds[0, ~live] = 1.0, math.inf, 0
        status, tsq = batch.update(kinds, grads, beta0)
        stop = live & ((status[0] != 0) | (tsq[0] < TOL))
        niter[stop] = it
        live &= ~stop
    return time.perf_counter() - t0, niter, gamma, x_best


def plain_rates(pkg, sb, n, B, seconds):
    """(c): updates/s of the streamed engine on B spaces from the identity, central cuts resident in HBM, K = 1 and K = 8"""
    batch = batch_class(pkg).new_with_scalar(np.ones(B), np.zeros((B, n)), device=0)
    dev = sb.DevArrays(pkg, B, n, np.random.default_rng(n))
    out = {}
    try:
        for K in (1, sb.KMAX):
            out[K] = sb.window(lambda: dev.launch(batch, K), batch.synchronize, K * B, seconds)
            dev.check_status(K, f"plain update, K = {K}")
    finally:
        dev.free()
    return out


def bench(pkg, ref, svb, sb, nfeat, m, B, max_iters, args):
    n = nfeat + 1
    svb.MAX_ITERS, svb.TOL, svb.STABLE = max_iters, TOL, STABLE   # tools/batch_svm_bench.py: cpu_run reads them
    data_d, lab_d = svb.problems(ref, m, nfeat, args.distinct, args.shared)
    D = lab_d.shape[0]
    if not args.shared:
        B = max(D, min(B, int(args.table_cap_gib * (1 << 30)) // (8 * m * nfeat)))
    cpu, c_niter, c_gamma, c_x = svb.cpu_run(data_d, lab_d, args.shared)
    data, lab = svb.tiled(data_d, lab_d, B, args.shared)
    prob = pkg.BatchSvmProblem.streamed(data, lab, device=0)
    del data
    times = []
    for rep in range(args.warmup + args.reps):
        dt, x_best, niter, gamma = device_run(pkg, prob, max_iters)
        if rep >= args.warmup:
            times.append(dt)
    which = np.arange(B) % D
    bits = svb.bits
    assert np.array_equal(niter, c_niter[which]), "device and CPU disagree (niter)"
    assert np.array_equal(bits(gamma), bits(c_gamma[which])), "device and CPU disagree (gamma)"
    assert np.array_equal(bits(x_best), bits(c_x[which])), "device and CPU disagree (x_best)"
    host_run(pkg, prob, min(3, max_iters))   # (warm-up: the wide assess kernel's first launch)
    host_s, niter_h, gamma_h, x_h = host_run(pkg, prob, max_iters)
    assert np.array_equal(niter_h, niter), "device and host-driven form disagree (niter)"
    assert np.array_equal(bits(gamma_h), bits(gamma)), "device and host-driven form disagree (gamma)"
    assert np.array_equal(bits(x_h), bits(x_best)), "device and host-driven form disagree (x_best)"
    del prob
    plain = plain_rates(pkg, sb, n, B, args.seconds)
    ran = np.where(niter < max_iters, niter + 1, niter)   # rounds per problem; a launch lasts as long as its longest member
    rounds = int(np.sum(ran))
    med = statistics.median(times)
    rate = rounds / med
    host_rate = rounds / host_s
    matrix = (24.0 if STABLE else 16.0) * n * n
    model = matrix + 8.0 * nfeat * m + 4.0 * m
    return {"bench": "batch_svm_streamed", "space": "stable" if STABLE else "ell", "nfeat": nfeat, "n": n, "m": m, "B": B,
            "table": "shared" if args.shared else "per-problem", "distinct": D, "max_iters": max_iters, "rounds": rounds,
            "device_s": {"median": med, "min": min(times), "max": max(times), "reps": len(times)},
            "niter_min": int(niter.min()), "niter_max": int(niter.max()),
            "device_rounds_per_s": rate, "s_per_round": med / int(ran.max()),
            "cpu_rounds_per_s": cpu["iters_per_s"], "over_cpu_one_thread": rate / cpu["iters_per_s"],
            "host_s": host_s, "host_rounds_per_s": host_rate, "over_host": rate / host_rate,
            "plain_updates_per_s_K1": plain[1], "plain_updates_per_s_K8": plain[sb.KMAX],
            "over_plain_K1": rate / plain[1], "over_plain_K8": rate / plain[sb.KMAX],
            "model_bytes_per_round": model, "model_matrix_share": matrix / model, "model_GB_per_s": rate * model / 1e9,
            "fold_chain": -(-m // n) * nfeat}


def oracle_share(lines):
    """seconds per round of the longest member = t0 + c m over the shapes of one n: the share c m / (t0 + c m) per shape"""
    ms = np.array([l["m"] for l in lines], dtype=np.float64)
    ts = np.array([l["s_per_round"] for l in lines])
    c, t0 = np.polyfit(ms, ts, 1)
    return {"bench": "batch_svm_streamed_oracle_share", "space": lines[0]["space"], "n": lines[0]["n"], "B": [l["B"] for l in lines],
            "s_per_round_at_m_0": t0, "s_per_round_per_sample": c,
            "share": {str(l["m"]): c * l["m"] / (t0 + c * l["m"]) for l in lines}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--space", choices=("ell", "stable"), default="ell")
    ap.add_argument("--shared", action="store_true", help="one table for every problem")
    ap.add_argument("--nfeat", default="128,255,511,1023")
    ap.add_argument("--m-over-n", default="0.5,2,8")
    ap.add_argument("--batches", default=None, help="B per nfeat; default 1536,1536,768,256 (--space stable: 1536,512,512,512)")
    ap.add_argument("--iters", default="1500,600,200,60", help="max_iters per nfeat")
    ap.add_argument("--distinct", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0.5, help="window of the plain update rate")
    ap.add_argument("--table-cap-gib", type=float, default=4.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    global STABLE
    STABLE = args.space == "stable"
    nfeats = [int(v) for v in args.nfeat.split(",")]
    if args.batches is None:
        args.batches = "1536,512,512,512" if STABLE else "1536,1536,768,256"
    batches = [int(v) for v in args.batches.split(",")]
    iters = [int(v) for v in args.iters.split(",")]
    if not len(nfeats) == len(batches) == len(iters):
        raise SystemExit("--nfeat, --batches and --iters must have the same length")
    import ellalgo_rs_amd as pkg
    import batch_streamed_bench as sb
    import batch_svm_bench as svb
    import batch_svm_reference as ref
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched svm loop has no CPU path")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for nfeat, B, max_iters in zip(nfeats, batches, iters):
        lines = []
        for ratio in (float(v) for v in args.m_over_n.split(",")):
            lines.append(bench(pkg, ref, svb, sb, nfeat, max(1, int(round(ratio * (nfeat + 1)))), B, max_iters, args))
            emit(lines[-1])
        if len(lines) > 1:
            emit(oracle_share(lines))


if __name__ == "__main__":
    main()
