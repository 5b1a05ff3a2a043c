"""CPU: the creation-time defaults of every option key of include/ellhip.h (ellhip_set_default_option /
ellhip_default_option need no device): factory values, the allowed values at their edges, refusals that leave the stored
value alone, and the three per-handle-only keys."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# key -> (factory value, allowed values): (lo, hi) is a range (hi None: no upper bound), a list is a set -- as documented in
# the table of include/ellhip.h
DEFAULTS = {
    "AUTO_DEFER": (1, (0, 1)), "SYMV": (1, (0, 1)), "SYMV_MIN_N": (5120, (512, None)), "APPLY_LOWER": (1, (0, 1)),
    "APPLY_KERNEL": (-1, (-1, 2)), "FUSE_DOTS": (1, (0, 1)), "STABLE_SOLVE": (3, (0, 3)), "STABLE_FACTOR": (2, (0, 2)),
    "PAD": (-1, (-1, 4096)), "LP_GRID": (0, (0, 65536)), "LP_WIDE": (-1, (-1, 1)), "BATCH_THREADS": (0, [0, 64, 128, 256]),
    "RESIDENT": (1, (0, 2)), "OVERLAP": (1, (0, 2)), "LOOKAHEAD": (32, (1, 32)), "QUEUE_DEPTH": (48, [0, 48]),
    "STAGE_DIRECT": (1, (0, 1)), "APPLY_SYMM": (1, (0, 1)), "PACKED_OPERANDS": (1, (0, 1)),
}
HANDLE_ONLY = ["RESIDENT_FAULT", "RESIDENT_ABANDONED", "STABLE_MIRRORED"]   # keys 17, 18, 19


def header_options():
    text = open(os.path.join(ROOT, "include", "ellhip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define ELLHIP_OPT_([A-Z0-9_]+) (\d+)\b", text, re.M)}


def values_of(allowed):
    """(values to set and read back: lowest, highest, one interior; the first values outside the allowed set)"""
    if isinstance(allowed, list):
        inside = [allowed[0], allowed[-1], allowed[len(allowed) // 2]]
        outside = sorted({v + d for v in allowed for d in (-1, 1)} - set(allowed))
        return inside, outside
    lo, hi = allowed
    if hi is None:
        return [lo, 2 ** 40, lo + 1], [lo - 1]
    return [lo, hi, (lo + hi) // 2], [lo - 1, hi + 1]


@pytest.fixture(scope="module")
def lib():
    import ellalgo_rs_amd as pkg
    return pkg.capi.load()


def get(lib, key):
    v = C.c_int64(-12345)
    rc = lib.ellhip_default_option(key, C.byref(v))
    return rc, v.value


def test_the_table_covers_every_key_of_the_header():
    assert set(DEFAULTS) | set(HANDLE_ONLY) == set(header_options()) and not set(DEFAULTS) & set(HANDLE_ONLY)
    assert [header_options()[k] for k in HANDLE_ONLY] == [17, 18, 19]


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_default_value_edges_and_refusals(lib, name):
    from ellalgo_rs_amd import capi
    key = header_options()[name]
    factory, allowed = DEFAULTS[name]
    assert get(lib, key) == (0, factory)
    inside, outside = values_of(allowed)
    try:
        for v in inside:
            assert lib.ellhip_set_default_option(key, v) == 0, (name, v)
            assert get(lib, key) == (0, v)
        for v in outside:
            before = get(lib, key)[1]
            assert lib.ellhip_set_default_option(key, v) == capi.E_INVALID, (name, v)
            assert lib.ellhip_last_error()   # a message, whatever its text
            assert get(lib, key) == (0, before), (name, v)
    finally:
        assert lib.ellhip_set_default_option(key, factory) == 0   # (also the two keys conftest.py's list does not cover)
    assert get(lib, key) == (0, factory)


@pytest.mark.parametrize("name", ["RESIDENT_ABANDONED", "STABLE_MIRRORED"])
def test_read_only_keys_have_no_default(lib, name):
    from ellalgo_rs_amd import capi
    key = header_options()[name]
    for v in (-1, 0, 1):
        assert lib.ellhip_set_default_option(key, v) == capi.E_INVALID
    assert get(lib, key)[0] == capi.E_INVALID


def test_the_test_hook_has_no_default(lib):
    """ELLHIP_OPT_RESIDENT_FAULT is per handle only: both defaults calls refuse it (set_default used to accept the value,
    store nothing and return 0)."""
    from ellalgo_rs_amd import capi
    key = header_options()["RESIDENT_FAULT"]
    for v in (-2, -1, 0, 7):
        assert lib.ellhip_set_default_option(key, v) == capi.E_INVALID
    assert get(lib, key)[0] == capi.E_INVALID


def test_unknown_keys_and_null_are_refused(lib):
    from ellalgo_rs_amd import capi
    for key in (0, 23, -1, 1000):
        assert lib.ellhip_set_default_option(key, 0) == capi.E_INVALID
        assert get(lib, key)[0] == capi.E_INVALID
    assert lib.ellhip_default_option(header_options()["SYMV"], None) == capi.E_INVALID
