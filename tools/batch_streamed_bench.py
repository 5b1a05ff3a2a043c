#!/usr/bin/env python3
"""Throughput of the streamed batch engine (include/ellhip_batch_streamed.h).

Shapes.  For each n: B `Ell` spaces from the identity, central cuts with seeded normal gradients (they always succeed; every
status of the last launch of each window is checked), K = 1 and K = 8 cuts per launch, every input resident in HBM
(ellhip_batch_update_dev).  Two populations per n: B * 8 n^2 ~ 64 MiB (the matrices fit the 256 MiB Infinity Cache; such
lines carry "infinity_cache_resident": true) and ~ 4 GiB (beyond it).

Method.  Each form is warmed up, then timed over a window of at least --seconds of wall clock that ends in a synchronise;
the window is repeated --reps times with the forms ALTERNATING (streamed K = 1, streamed K = 8, then the baselines), and the
median, min and max of the repetitions are reported.  Rates are whole-launch figures (launch, cut inputs, scalar stage and
matrix passes together), not a kernel's share.  bytes_per_update is this tool's byte model of what the kernel moves,
((16 K + 8) n^2 + K (8 n + 24) + 16 n + 24) / K per ellipsoid, and hbm_peak_frac is that rate over the 8.0 TB/s HBM3E peak.

Baselines (large population only; code the streamed engine does not touch), on the same cuts: 16 single `Ell` handles of
the same n that receive the cuts of ellipsoids 0..15, driven one after another, once with one ellhip_update per cut (compare
with K = 1) and once with one ellhip_queue_run of 8 uploaded cuts per handle (compare with K = 8); at n <= 128 also the LDS
engine (ellhip_batch_create) on the same population.  Before any rate is printed, 8 cuts are applied to 16 ellipsoids by
every form from fresh handles and the states (Q, xc, kappa) must agree with the streamed batch within 1e-10 (relative,
inf-norm); the LDS engine must agree to the bit.

    python3 tools/batch_streamed_bench.py [--sizes 128,129,256,512,1024] [--seconds 1.0] [--reps 3] [--out F]

--space stable measures EllStable on the same engine (include/ellhip_batch_streamed_stable.h) instead:
for each n of --sizes (default 256,512,1024) and each B of --batches (default 64,512), B `EllStable` spaces from the identity,
the same central cuts, K = 8 per launch.  Three forms alternate inside every repetition: the streamed EllStable batch, the
streamed Ell batch of the same shape (for scale), and the baseline -- 16 single `EllStable` handles of the same n that receive
the cuts of ellipsoids 0..15 through ellhip_update, one after another (what B spaces of this size had to use before; its rate
per update does not depend on how many handles take turns, except that 16 of them stay in the Infinity Cache where B = 512
would not, which favours the baseline).  bytes_per_update is the byte model of a successful cut, 24 n^2 + 48 n + 24: the factor
read 4 n^2, the scratch triangle written 4 n^2 and read twice 8 n^2, the factor read and written 8 n^2.  Before any rate, 8 cuts
on 16 ellipsoids by the batch and by the single handles must agree within 1e-10 in xc, kappa, the diagonal and the factor.

    python3 tools/batch_streamed_bench.py --space stable [--sizes 256,512,1024] [--batches 64,512] [--out F]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KMAX = 8
NSINGLE = 16
HBM_PEAK_BS = 8.0e12
POPULATIONS = (("64MiB", 64 << 20, True), ("4GiB", 4 << 30, False))
TOL = 1e-10


def rel_inf(a, b):
    d = float(np.max(np.abs(a - b)))
    s = float(np.max(np.abs(b)))
    return 0.0 if d == 0.0 else (d / s if s > 0 else np.inf)


class DevArrays:
    """the cut arrays of one population in HBM: kinds, grads, beta0, has_beta1, beta1 [KMAX][B], and a status array"""

    def __init__(self, pkg, B, n, rng):
        self.hip = C.CDLL(sorted(pkg.capi.mapped_runtimes()["libamdhip64"])[0])  # the runtime the engine is bound to
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.B = B
        self.grads = rng.standard_normal((KMAX, B, n))
        self.status = np.full((KMAX, B), -1, dtype=np.int32)
        host = [np.full((KMAX, B), 1, dtype=np.int32), self.grads, np.zeros((KMAX, B)), np.zeros((KMAX, B), dtype=np.int32),
                np.zeros((KMAX, B)), self.status]
        self.ptrs = []
        for x in host:
            p = C.c_void_p()
            if self.hip.hipMalloc(C.byref(p), x.nbytes) != 0:
                raise RuntimeError("hipMalloc failed")
            self.ptrs.append(p)
            if self.hip.hipMemcpy(p, x.ctypes.data, x.nbytes, 1) != 0:
                raise RuntimeError("hipMemcpy failed")

    def launch(self, batch, K):
        batch.update_dev(K, *self.ptrs[:5], self.ptrs[5], None)

    def check_status(self, K, what):
        if self.hip.hipMemcpy(self.status.ctypes.data, self.ptrs[5], self.status.nbytes, 2) != 0:
            raise RuntimeError("hipMemcpy failed")
        if not (self.status[:K] == 0).all():
            raise RuntimeError(f"{what}: a central cut did not succeed")

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def window(step, sync, per_step, seconds):
    """updates/s of `step` repeated for at least `seconds`, the window ending in `sync`"""
    step()
    sync()
    t0 = time.perf_counter()
    step()
    sync()
    one = max(time.perf_counter() - t0, 1e-6)
    steps = max(2, int(np.ceil(seconds / one)))
    while True:
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        elapsed = time.perf_counter() - t0
        if elapsed >= seconds:
            return steps * per_step / elapsed
        steps = int(np.ceil(steps * 1.3 * seconds / elapsed))


def single_handles(pkg, n, grads16):
    """16 single Ell handles and the two ways of driving them with the 8 cuts of ellipsoids 0..15"""
    upd = [pkg.Ell.new_with_scalar(1.0, np.zeros(n)) for _ in range(NSINGLE)]
    que = [pkg.Ell.new_with_scalar(1.0, np.zeros(n)) for _ in range(NSINGLE)]
    for h, s in enumerate(que):
        s.queue_upload(np.full(KMAX, 1, dtype=np.int32), grads16[:, h], np.zeros(KMAX))

    def step_update():
        for k in range(KMAX):
            for h, s in enumerate(upd):
                if int(s._update(1, (grads16[k, h], 0.0))) != 0:
                    raise RuntimeError("ellhip_update: a central cut did not succeed")

    def step_queue():
        for s in que:
            s.queue_run(0, KMAX)

    def sync_queue():
        for s in que:
            s.synchronize()
            st, _ = s.queue_results()
            if not (st == 0).all():
                raise RuntimeError("ellhip_queue_run: a central cut did not succeed")

    return upd, que, step_update, step_queue, sync_queue


def verify(pkg, n, grads16):
    """8 cuts on 16 ellipsoids by every form from fresh handles: states within TOL of the streamed batch (K = 8)"""
    z = np.zeros((NSINGLE, n))
    kinds = np.full((KMAX, NSINGLE), 1, dtype=np.int32)
    b0 = np.zeros((KMAX, NSINGLE))
    ref = pkg.EllBatchStreamed.new_with_scalar(1.0, z)
    st, _ = ref.update(kinds, grads16, b0)
    one = pkg.EllBatchStreamed.new_with_scalar(1.0, z)
    for k in range(KMAX):
        s1, _ = one.update(kinds[k], grads16[k], b0[k])
        st = np.concatenate([st, s1])
    if not (st == 0).all():
        raise RuntimeError("verify: a central cut did not succeed")
    q, x, kap = ref.mq, ref.xc(), ref.kappa
    worst = {"streamed_k1": max(rel_inf(one.mq, q), rel_inf(one.xc(), x), rel_inf(one.kappa, kap))}
    upd, que, step_update, step_queue, sync_queue = single_handles(pkg, n, grads16)
    step_update()
    step_queue()
    sync_queue()
    for name, hs in (("ellhip_update", upd), ("ellhip_queue_run", que)):
        worst[name] = max(max(rel_inf(s.mq, q[h]), rel_inf(s.xc(), x[h]), abs(s.kappa - kap[h]) / abs(kap[h]))
                          for h, s in enumerate(hs))
    if n <= 128:
        lds = pkg.EllBatch.new_with_scalar(1.0, z)
        lds.update(kinds, grads16, b0)
        if not (np.array_equal(lds.mq, q) and np.array_equal(lds.xc(), x) and np.array_equal(lds.kappa, kap)):
            raise RuntimeError("verify: the LDS engine and the streamed engine differ in a bit")
        worst["lds_engine"] = 0.0
    bad = {k: v for k, v in worst.items() if not v <= TOL}
    if bad:
        raise RuntimeError(f"verify n={n}: states differ from the streamed batch by more than {TOL}: {bad}")
    return worst


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def bytes_per_update(n, K):
    return ((16.0 * K + 8.0) * n * n + K * (8.0 * n + 24.0) + 16.0 * n + 24.0) / K


def run_population(pkg, n, name, nbytes, cached, args, emit):
    B = max(NSINGLE, int(round(nbytes / (8.0 * n * n))))
    rng = np.random.default_rng(0x5EED + n)
    dev = DevArrays(pkg, B, n, rng)
    try:
        grads16 = np.ascontiguousarray(dev.grads[:, :NSINGLE])
        worst = verify(pkg, n, grads16)
        forms = {}
        batch = pkg.EllBatchStreamed.new_with_scalar(1.0, np.zeros((B, n)))
        for K in (1, KMAX):
            forms[f"streamed_k{K}"] = (lambda K=K: dev.launch(batch, K), batch.synchronize, K * B, K)
        lds = None
        if not cached:
            upd, que, step_update, step_queue, sync_queue = single_handles(pkg, n, grads16)
            forms["sequential_ellhip_update"] = (step_update, lambda: None, KMAX * NSINGLE, 1)
            forms["sequential_queue_run_8"] = (step_queue, sync_queue, KMAX * NSINGLE, KMAX)
            if n <= 128:
                lds = pkg.EllBatch.new_with_scalar(1.0, np.zeros((B, n)))
                for K in (1, KMAX):
                    forms[f"lds_engine_k{K}"] = (lambda K=K: dev.launch(lds, K), lds.synchronize, K * B, K)
        rates = {f: [] for f in forms}
        for _ in range(args.reps):
            for f, (step, sync, per_step, K) in forms.items():  # the forms alternate inside every repetition
                rates[f].append(window(step, sync, per_step, args.seconds))
                if f.startswith(("streamed", "lds")):
                    dev.check_status(K, f)
        if not np.isfinite(batch.tsq()).all():
            raise RuntimeError(f"n={n}: non-finite tsq")
        for K in (1, KMAX):
            r = stats(rates[f"streamed_k{K}"])
            bpu = bytes_per_update(n, K)
            rec = {"workload": f"ell-batch-streamed-n{n}-{name}-k{K}", "n": n, "ellipsoids": B, "cuts_per_launch": K,
                   "population_bytes": B * 8 * n * n, "infinity_cache_resident": cached,
                   "updates_per_s": r, "bytes_per_update": bpu, "byte_model_bytes_per_s": bpu * r["median"],
                   "hbm_peak_frac": bpu * r["median"] / HBM_PEAK_BS,
                   "figure": "whole launch (wall clock, inputs resident, ellhip_batch_update_dev), not a kernel's share",
                   "window_seconds": args.seconds, "repetitions": args.reps, "cuts": "central, seeded normal gradients",
                   "verified_rel_err": worst}
            if not cached:
                base = "sequential_ellhip_update" if K == 1 else "sequential_queue_run_8"
                b = stats(rates[base])
                rec["baseline"] = {"form": base + f" ({NSINGLE} single Ell handles, one after another)", "updates_per_s": b}
                rec["ratio_vs_baseline"] = r["median"] / b["median"]
                if lds is not None:
                    l = stats(rates[f"lds_engine_k{K}"])
                    rec["lds_engine"] = {"updates_per_s": l}
                    rec["ratio_vs_lds_engine"] = r["median"] / l["median"]
            emit(rec)
    finally:
        dev.free()


def stable_singles(pkg, n, grads16):
    """16 single EllStable handles and the step that gives each the 8 cuts of its ellipsoid through ellhip_update"""
    hs = [pkg.EllStable.new_with_scalar(1.0, np.zeros(n)) for _ in range(NSINGLE)]

    def step():
        for k in range(KMAX):
            for h, s in enumerate(hs):
                if int(s._update(1, (grads16[k, h], 0.0))) != 0:
                    raise RuntimeError("ellhip_update: a central cut did not succeed")

    return hs, step


def verify_stable(pkg, n, grads16):
    """8 cuts on 16 ellipsoids by the streamed EllStable batch (K = 8 and K = 1) and by single handles from fresh state"""
    z = np.zeros((NSINGLE, n))
    kinds = np.full((KMAX, NSINGLE), 1, dtype=np.int32)
    b0 = np.zeros((KMAX, NSINGLE))
    ref = pkg.EllStableBatchStreamed.new_with_scalar(1.0, z)
    st, _ = ref.update(kinds, grads16, b0)
    one = pkg.EllStableBatchStreamed.new_with_scalar(1.0, z)
    for k in range(KMAX):
        s1, _ = one.update(kinds[k], grads16[k], b0[k])
        st = np.concatenate([st, s1])
    if not (st == 0).all():
        raise RuntimeError("verify: a central cut did not succeed")
    q, x, kap = ref.mq, ref.xc(), ref.kappa
    if not (np.array_equal(one.mq, q) and np.array_equal(one.xc(), x) and np.array_equal(one.kappa, kap)):
        raise RuntimeError("verify: K = 1 and K = 8 differ in a bit")
    hs, step = stable_singles(pkg, n, grads16)
    step()
    worst = {"ellhip_update": max(max(rel_inf(np.triu(s.mq), np.triu(q[h])), rel_inf(s.xc(), x[h]),
                                      abs(s.kappa - kap[h]) / abs(kap[h])) for h, s in enumerate(hs))}
    if not worst["ellhip_update"] <= TOL:
        raise RuntimeError(f"verify n={n}: single EllStable handles differ from the streamed batch by more than {TOL}: {worst}")
    return worst


def run_stable(pkg, n, B, args, emit):
    rng = np.random.default_rng(0x5EED + n)
    dev = DevArrays(pkg, B, n, rng)
    try:
        grads16 = np.ascontiguousarray(dev.grads[:, :NSINGLE])
        worst = verify_stable(pkg, n, grads16)
        stable = pkg.EllStableBatchStreamed.new_with_scalar(1.0, np.zeros((B, n)))
        ell = pkg.EllBatchStreamed.new_with_scalar(1.0, np.zeros((B, n)))
        hs, step = stable_singles(pkg, n, grads16)
        forms = {"streamed_stable_k8": (lambda: dev.launch(stable, KMAX), stable.synchronize, KMAX * B),
                 "streamed_ell_k8": (lambda: dev.launch(ell, KMAX), ell.synchronize, KMAX * B),
                 "sequential_ellhip_update": (step, lambda: None, KMAX * NSINGLE)}
        rates = {f: [] for f in forms}
        for _ in range(args.reps):
            for f, (go, sync, per_step) in forms.items():  # the forms alternate inside every repetition
                rates[f].append(window(go, sync, per_step, args.seconds))
                if f.startswith("streamed"):
                    dev.check_status(KMAX, f)
        if not (np.isfinite(stable.tsq()).all() and np.isfinite(ell.tsq()).all()):
            raise RuntimeError(f"n={n}: non-finite tsq")
        r, e, b = (stats(rates[f]) for f in forms)
        bpu = 24.0 * n * n + 48.0 * n + 24.0
        emit({"workload": f"ellstable-batch-streamed-n{n}-b{B}-k{KMAX}", "n": n, "ellipsoids": B, "cuts_per_launch": KMAX,
              "population_bytes": B * 8 * n * n, "updates_per_s": r, "bytes_per_update": bpu,
              "byte_model_bytes_per_s": bpu * r["median"], "hbm_peak_frac": bpu * r["median"] / HBM_PEAK_BS,
              "streamed_ell": {"updates_per_s": e}, "ratio_vs_streamed_ell": r["median"] / e["median"],
              "baseline": {"form": f"sequential_ellhip_update ({NSINGLE} single EllStable handles, one after another)",
                           "updates_per_s": b},
              "ratio_vs_baseline": r["median"] / b["median"],
              "figure": "whole launch (wall clock, inputs resident, ellhip_batch_update_dev), not a kernel's share",
              "window_seconds": args.seconds, "repetitions": args.reps, "cuts": "central, seeded normal gradients",
              "verified_rel_err": worst})
    finally:
        dev.free()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--space", choices=("ell", "stable"), default="ell")
    ap.add_argument("--batches", default="64,512", help="--space stable: ellipsoids per batch")
    ap.add_argument("--sizes", default=None, help="default 128,129,256,512,1024 (--space stable: 256,512,1024)")
    ap.add_argument("--seconds", type=float, default=1.0, help="length of a timed window (at least)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--populations", default="64MiB,4GiB")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.reps < 3 or args.seconds < 1.0:
        print("note: fewer than 3 repetitions or windows under a second are for trying the tool out, not for quoting",
              file=sys.stderr)
    import ellalgo_rs_amd as pkg
    pkg.capi.load()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    if args.sizes is None:
        args.sizes = "256,512,1024" if args.space == "stable" else "128,129,256,512,1024"
    if args.space == "stable":
        for n in (int(s) for s in args.sizes.split(",")):
            for B in (int(s) for s in args.batches.split(",")):
                run_stable(pkg, n, max(B, NSINGLE), args, emit)
        return
    for n in (int(s) for s in args.sizes.split(",")):
        for name, nbytes, cached in POPULATIONS:
            if name in args.populations.split(","):
                run_population(pkg, n, name, nbytes, cached, args, emit)


if __name__ == "__main__":
    main()
