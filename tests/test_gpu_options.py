"""GPU: ellhip_set_option / ellhip_get_option key by key on two handles of n = 8 (one Ell, one EllStable): who may set what,
the allowed values, what reads back, what a new handle and a clone start with."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 8
# key -> (values that round-trip, values that are refused)
ELL_KEYS = {
    "SYMV": ([0, 1], [-1, 2]), "SYMV_MIN_N": ([512, 513, 2 ** 40, 5120], [511, 0, -1]), "APPLY_LOWER": ([0, 1], [-1, 2]),
    "APPLY_KERNEL": ([2, 0, 1, -1], [-2, 3]), "FUSE_DOTS": ([0, 1], [-1, 2]), "RESIDENT": ([0, 2, 1], [-1, 3]),
    "OVERLAP": ([0, 2, 1], [-1, 3]), "LOOKAHEAD": ([1, 17, 32], [0, 33]), "QUEUE_DEPTH": ([0, 48], [-1, 1, 24, 47, 49]),
    "APPLY_SYMM": ([0, 1], [-1, 2]), "PACKED_OPERANDS": ([0, 1], [-1, 2]), "RESIDENT_FAULT": ([0, 5, 2 ** 40, -1], [-2]),
}
STABLE_KEYS = {"STABLE_SOLVE": ([0, 1, 2, 3], [-1, 4]), "STABLE_FACTOR": ([0, 1, 2], [-1, 3])}
DEFAULT_ONLY = {"AUTO_DEFER": 0, "PAD": 8, "LP_GRID": 4, "LP_WIDE": 0, "BATCH_THREADS": 64, "STAGE_DIRECT": 0}
THIRTEEN = ["SYMV", "SYMV_MIN_N", "APPLY_LOWER", "APPLY_KERNEL", "FUSE_DOTS", "RESIDENT", "OVERLAP", "LOOKAHEAD", "QUEUE_DEPTH",
            "APPLY_SYMM", "PACKED_OPERANDS", "STABLE_SOLVE", "STABLE_FACTOR"]
FACTORY = dict(zip(THIRTEEN, [1, 5120, 1, -1, 1, 1, 1, 32, 48, 1, 1, 3, 2]))
OTHER = dict(zip(THIRTEEN, [0, 1024, 0, 1, 0, 2, 2, 4, 0, 0, 0, 1, 1]))   # allowed, and none a factory value


def key(pkg, name):
    return getattr(pkg.capi, "OPT_" + name)


def get(pkg, h, name):
    v = C.c_int64(-12345)
    rc = pkg.capi.load().ellhip_get_option(h._h, key(pkg, name), C.byref(v))
    return rc, v.value


def put(pkg, h, name, value):
    return pkg.capi.load().ellhip_set_option(h._h, key(pkg, name), value)


@pytest.fixture(scope="module")
def handles(gpu):
    return gpu.Ell.new_with_scalar(1.0, np.zeros(N), device=0), gpu.EllStable.new_with_scalar(1.0, np.zeros(N), device=0)


@pytest.mark.parametrize("name", sorted(ELL_KEYS))
def test_ell_keys_round_trip_on_ell_only(gpu, handles, name):
    ell, stable = handles
    good, bad = ELL_KEYS[name]
    start_stable = get(gpu, stable, name)
    assert start_stable[0] == 0   # get_option does not look at the variant
    for v in good:
        assert put(gpu, ell, name, v) == 0, (name, v)
        assert get(gpu, ell, name) == (0, v)
        for w in bad:
            assert put(gpu, ell, name, w) == gpu.capi.E_INVALID, (name, w)
            assert get(gpu, ell, name) == (0, v), (name, w)
        assert put(gpu, stable, name, v) == gpu.capi.E_INVALID, (name, v)
    assert get(gpu, stable, name) == start_stable


@pytest.mark.parametrize("name", sorted(STABLE_KEYS))
def test_stable_keys_round_trip_on_ellstable_only(gpu, handles, name):
    ell, stable = handles
    good, bad = STABLE_KEYS[name]
    start_ell = get(gpu, ell, name)
    assert start_ell == (0, FACTORY[name])
    for v in good:
        assert put(gpu, stable, name, v) == 0, (name, v)
        assert get(gpu, stable, name) == (0, v)
        for w in bad:
            assert put(gpu, stable, name, w) == gpu.capi.E_INVALID, (name, w)
            assert get(gpu, stable, name) == (0, v), (name, w)
        assert put(gpu, ell, name, v) == gpu.capi.E_INVALID, (name, v)
    assert get(gpu, ell, name) == start_ell
    assert put(gpu, stable, name, FACTORY[name]) == 0


def test_default_only_and_read_only_keys(gpu, handles):
    for h in handles:
        for name, v in DEFAULT_ONLY.items():
            assert put(gpu, h, name, v) == gpu.capi.E_INVALID, name
        for name in ("AUTO_DEFER", "LP_GRID", "LP_WIDE", "BATCH_THREADS"):
            assert get(gpu, h, name)[0] == gpu.capi.E_INVALID, name
        assert get(gpu, h, "PAD") == (0, 0)          # n = 8: dense rows
        assert get(gpu, h, "STAGE_DIRECT")[0] == 0 and get(gpu, h, "STAGE_DIRECT")[1] in (0, 1)
        assert get(gpu, h, "RESIDENT_ABANDONED") == (0, 0)
        assert get(gpu, h, "STABLE_MIRRORED")[0] == 0 and get(gpu, h, "STABLE_MIRRORED")[1] in (0, 1)
        for name in ("RESIDENT_ABANDONED", "STABLE_MIRRORED"):
            for v in (0, 1):
                assert put(gpu, h, name, v) == gpu.capi.E_INVALID, name
        assert gpu.capi.load().ellhip_set_option(h._h, 0, 0) == gpu.capi.E_INVALID
        assert gpu.capi.load().ellhip_set_option(h._h, 23, 0) == gpu.capi.E_INVALID
    with gpu.capi.default_options({gpu.capi.OPT_PAD: 4, gpu.capi.OPT_STAGE_DIRECT: 0}):
        h = gpu.Ell.new_with_scalar(1.0, np.zeros(N), device=0)
    assert get(gpu, h, "PAD") == (0, 4)              # reads ld - n
    assert get(gpu, h, "STAGE_DIRECT") == (0, 0)


def test_a_schedule_option_is_refused_inside_a_two_phase_update(gpu):
    lib = gpu.capi.load()
    h = gpu.Ell.new_with_scalar(1.0, np.zeros(N), device=0)
    g = np.ones(N)
    assert lib.ellhip_update_begin(h._h, 0, g.ctypes.data_as(C.c_void_p), 0.1, 0, 0.0) == 0
    assert put(gpu, h, "SYMV", 0) == gpu.capi.E_STATE
    assert get(gpu, h, "SYMV") == (0, 1)
    assert put(gpu, h, "SYMV", 2) == gpu.capi.E_INVALID   # the value is looked at first
    assert put(gpu, h, "LOOKAHEAD", 4) == 0               # read per queue run: legal at any point
    assert lib.ellhip_update_end(h._h) == 0
    assert put(gpu, h, "SYMV", 0) == 0 and get(gpu, h, "SYMV") == (0, 0)


def test_new_handles_and_clones_start_with_the_right_values(gpu):
    capi = gpu.capi
    try:
        for name in THIRTEEN:
            capi.set_default_option(key(gpu, name), OTHER[name])
        made = gpu.Ell.new_with_scalar(1.0, np.zeros(N), device=0), gpu.EllStable.new_with_scalar(1.0, np.zeros(N), device=0)
    finally:
        for name in THIRTEEN:   # (APPLY_SYMM and PACKED_OPERANDS are not in conftest.py's list)
            capi.set_default_option(key(gpu, name), FACTORY[name])
    for h in made:
        assert {name: get(gpu, h, name) for name in THIRTEEN} == {name: (0, OTHER[name]) for name in THIRTEEN}
    fresh = gpu.Ell.new_with_scalar(1.0, np.zeros(N), device=0)
    assert {name: get(gpu, fresh, name) for name in THIRTEEN} == {name: (0, FACTORY[name]) for name in THIRTEEN}
    # a clone: the source's thirteen (set per handle here where the variant allows it), not the test hook
    src = made[0]
    mixed = dict(OTHER, LOOKAHEAD=7, SYMV_MIN_N=2048, RESIDENT=0, APPLY_KERNEL=2)
    for name in THIRTEEN:
        if name not in STABLE_KEYS:
            assert put(gpu, src, name, mixed[name]) == 0
    assert put(gpu, src, "RESIDENT_FAULT", 3) == 0
    twin = src.clone()
    assert {name: get(gpu, twin, name) for name in THIRTEEN} == {name: (0, mixed[name]) for name in THIRTEEN}
    assert get(gpu, src, "RESIDENT_FAULT") == (0, 3) and get(gpu, twin, "RESIDENT_FAULT") == (0, -1)
    stwin = made[1].clone()
    assert {name: get(gpu, stwin, name) for name in THIRTEEN} == {name: (0, OTHER[name]) for name in THIRTEEN}
