#!/bin/bash
# Tuning builds of the scalar stage's slice length (run on the GPU box; the box is scratch).
O=$(mktemp -d)
for sl in 1024 512 256; do
  ELLHIP_EXTRA_HIPCC_FLAGS="-DELLHIP_SCALAR_SLICE=$sl" python -c "
import importlib, sys
sys.path.insert(0, '.')
b = importlib.import_module('ellalgo-rs_amd.build'); b.build(force=True)" || exit 1
  for w in n4096-deep n8192-deep n16384-parallel; do
    timeout -k 10 200 python bench.py --full --workload $w --no-cpu-baseline --host-path-steps 0 --compare-steps 0 > $O/slice.json 2> $O/slice.err || { tail -3 $O/slice.err; continue; }
    echo "slice=$sl: $(python tools/show_bench.py $O/slice.json | head -1)"
  done
done
