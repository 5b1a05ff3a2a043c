"""Python mirror of the round-robin problem handle over large LMI blocks and of its device-resident cutting-plane loops
(include/ellhip_lmi_loop.h): `min c'x  s.t.  F_j(x) > 0` over J `LMIOracle` / `LMI0Oracle` blocks from lmi.py (or, without
c, the feasibility problem), with the oracle of tests/lmi_tests.rs:142-171 generalised to J blocks walked on the device and
an `Ell` / `EllStable` from ell.py as the search space.  Bit-identical to the same loop driven from the host."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ell import _f64, _p


class LmiLoopProblem:
    def __init__(self, blocks, c=None):
        """blocks: 1 .. 8 LMIOracle / LMI0Oracle objects with the same n on the same device (kept alive by this object;
        do not call them while one of the loops below is running); c: [n] or None (feasibility problem)."""
        self._lib = capi.load()
        self._blocks = list(blocks)
        self.J = len(self._blocks)
        handles = [getattr(b, "_h", None) for b in self._blocks]
        arr = (C.c_void_p * max(self.J, 1))(*[h.value if h else None for h in handles])
        n = getattr(self._blocks[0], "n", 0) if self._blocks else 0
        c = None if c is None else _f64(c, n)
        h = C.c_void_p()
        capi.check(self._lib.ellhip_lmi_loop_create(C.byref(h), C.cast(arr, C.c_void_p), self.J, _p(c)),
                   "ellhip_lmi_loop_create")
        self._h = h
        self.n = int(n)
        self.has_c = c is not None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ellhip_lmi_loop_destroy(h)

    @property
    def blocks(self):
        return tuple(self._blocks)

    @property
    def idx(self) -> int:
        """the round-robin cursor: the station visited last, -1 when new"""
        out = C.c_int()
        capi.check(self._lib.ellhip_lmi_loop_get_idx(self._h, C.byref(out)), "ellhip_lmi_loop_get_idx")
        return int(out.value)

    @idx.setter
    def idx(self, value: int) -> None:
        capi.check(self._lib.ellhip_lmi_loop_set_idx(self._h, int(value)), "ellhip_lmi_loop_set_idx")

    def assess_optim(self, x, gamma: float):
        """(g, beta, station, gamma): station < J a block cut, J the objective cut, J + 1 shrunk"""
        x = _f64(x, self.n)
        g = np.empty(self.n, dtype=np.float64)
        b, st, gm = C.c_double(), C.c_int(), C.c_double(gamma)
        capi.check(self._lib.ellhip_lmi_loop_assess_optim(self._h, _p(x), C.byref(gm), _p(g), C.byref(b), C.byref(st)),
                   "ellhip_lmi_loop_assess_optim")
        return g, b.value, int(st.value), gm.value

    def assess_feas(self, x):
        """None when every block passes, else (g, beta, station)"""
        x = _f64(x, self.n)
        g = np.empty(self.n, dtype=np.float64)
        b, st = C.c_double(), C.c_int()
        rc = capi.check(self._lib.ellhip_lmi_loop_assess_feas(self._h, _p(x), _p(g), C.byref(b), C.byref(st)),
                        "ellhip_lmi_loop_assess_feas")
        return None if rc == 0 else (g, b.value, int(st.value))

    # ---- device-resident driver loops
    def cutting_plane_optim(self, space, gamma: float, max_iters: int, tol: float):
        """(x_best or None, niter, gamma)"""
        xb = np.empty(self.n, dtype=np.float64)
        hb, ni, gm = C.c_int(), C.c_int64(), C.c_double(gamma)
        capi.check(self._lib.ellhip_lmi_loop_optim(space._h, self._h, C.byref(gm), int(max_iters), float(tol), _p(xb),
                                                   C.byref(hb), C.byref(ni)), "ellhip_lmi_loop_optim")
        return (xb if hb.value else None), int(ni.value), gm.value

    def cutting_plane_feas(self, space, max_iters: int, tol: float):
        """(x or None, niter)"""
        x = np.empty(self.n, dtype=np.float64)
        ok, ni = C.c_int(), C.c_int64()
        capi.check(self._lib.ellhip_lmi_loop_feas(space._h, self._h, int(max_iters), float(tol), _p(x), C.byref(ok),
                                                  C.byref(ni)), "ellhip_lmi_loop_feas")
        return (x if ok.value else None), int(ni.value)
