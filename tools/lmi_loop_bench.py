"""The device-resident cutting-plane loops over large LMI blocks (include/ellhip_lmi_loop.h) against the host-driven loop:
one JSON line per shape.

  python tools/lmi_loop_bench.py [--shapes feas:16:64:1,optim:8:70:2] [--iters 200] [--out FILE]

Both sides are timed from a compiled caller, tests/cpp/lmi_loop_runner.cpp (its `bench` mode), through the C++ mirror
ellalgo-rs_amd/host/ellhip/lmi_loop_hip.hpp:
  host_*     the generic drivers of cutting_plane.hpp with the walk on the host: per iteration the centre down, one
             synchronising ellhip_lmi_assess_feas per station visited, and the cut through ellhip_update -- what the
             library offered before the loop handle existed
  device_*   ellhip_lmi_loop_optim / _feas: the window of station slots per iteration, the host looking once per 64
Host clock around the whole loop call; median of 3 after a warm-up run; separate handles on each side, built from the
same matrices; a line is printed only when niter, x, gamma, tsq and the cursor agree bit for bit.  *_us_per_iter divides
by the oracle calls made (the stopping iteration included).

Shapes are form:n:m:J.  Data: a seeded LCG, symmetric F_jk in (-1.5, 1.5), B_j strictly diagonally dominant (so x = 0 is
strictly feasible); tol = 0.  The optimisation form starts from Ell::new_with_scalar(400, 0); the feasibility form scales
B by 1e-6 and starts at centre 6, so that the loop runs for hundreds of iterations before it finds a point.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# the issue's shapes: single-block feasibility, and two blocks plus the objective
DEFAULT_SHAPES = "feas:16:64:1,feas:24:300:1,feas:8:2048:1,optim:8:70:2,optim:24:300:2,optim:8:1057:2"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    args = ap.parse_args()
    import cpp_build
    exe = cpp_build.build_runner("lmi_loop_runner.cpp", "hip")
    rc = 0
    for shape in args.shapes.split(","):
        form, n, m, J = shape.split(":")
        r = subprocess.run([exe, "bench", n, m, J, form, str(args.iters)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(f"{shape}: runner failed ({r.returncode}): {r.stderr.strip()}", file=sys.stderr)
            rc = 1
            continue
        line = r.stdout.strip()
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
