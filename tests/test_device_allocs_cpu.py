"""CPU: the owner of every handle's device and pinned memory (csrc/device_allocs.hpp).

tests/cpp/device_allocs_check.cpp includes the header alone and defines the five runtime calls itself (over malloc, with a
live count and a "fail the k-th call" switch); it is built with AddressSanitizer + UBSan and run as a child process, so a
leak, a double free or a use after free in the owner fails the run.  The second test keeps the library's own code from
going around the owner."""
import os
import re
import subprocess

from cpp_build import CPP, HIP_HOST_FLAGS, OUT, ROOT, _newer

CSRC = os.path.join(ROOT, "ellalgo-rs_amd", "csrc")
HEADER = os.path.join(CSRC, "device_allocs.hpp")


def test_owner_rolls_back_frees_and_reuses():
    os.makedirs(OUT, exist_ok=True)
    src, exe = os.path.join(CPP, "device_allocs_check.cpp"), os.path.join(OUT, "device_allocs_check")
    if _newer(exe, [src, HEADER]):
        # (the sanitizer runtimes linked statically: the program needs nothing from its environment to start)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *HIP_HOST_FLAGS, "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and r.stdout.strip().endswith("device_allocs_check: ok"), (r.returncode, r.stdout, r.stderr)


def test_only_the_owner_calls_the_allocation_functions():
    calls = re.compile(r"\b(hipMalloc|hipHostMalloc|hipExtMallocWithFlags|hipFree|hipHostFree)\s*\(")
    found = {}
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name)).read()
        n = len(calls.findall(text))
        if n:
            found[name] = n
    assert set(found) == {"device_allocs.hpp"}, found
    assert found["device_allocs.hpp"] == 5, found   # one call of each, nothing else
