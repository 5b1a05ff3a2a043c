"""CPU: the workgroup -> (column block, pair) map of k_group_reduce_p (csrc/group_reduce_map.hpp) visits exactly the grid, each
(blk, p) once, in both forms, and heavy first never returns to a heavier column block.  The header is plain C++; a host program
(tests/cpp/group_reduce_map_check.cpp, g++) walks the very function the kernel calls."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_slot_of_the_grid_once(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "group_reduce_map_check.cpp")
    exe = str(tmp_path / "group_reduce_map_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    grids = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(grids) == 7 * 6 * 2, r.stdout[-2000:]
    for g in grids:
        assert g["outside"] == 0 and g["missed"] == 0 and g["twice"] == 0 and g["went_back"] == 0 and g["ok"], g
    assert {(g["gx"], g["gy"]) for g in grids if g["heavy_first"]} >= {(128, 16), (128, 8), (256, 16), (33, 15)}
    assert r.returncode == 0
