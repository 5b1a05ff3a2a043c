"""Python mirror of `SvmOracle` (src/oracles/svm_oracle.rs:4-58) over the C ABI of include/ellhip_svm.h: the table
lives on the GPU, feature-major.  Same method name and return shape as the reference's `OracleOptim` impl;
`cutting_plane_optim` runs the reference's driver loop (src/cutting_plane.rs:286-313) entirely on the device with an
`Ell` / `EllStable` from ell.py (dimension nfeat + 1) as the search space.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ell import SingleCut, _f64, _p


class SvmOracle:
    def __init__(self, data, labels, device: int = -1):
        """data: m x nfeat (row-major, float64); labels: m integers (stored as int32, converted `as f64`)."""
        self._lib = capi.load()
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim != 2:
            raise ValueError("data must be a 2-D m x nfeat array")
        self.m, self.nfeat = int(data.shape[0]), int(data.shape[1])
        self.n = self.nfeat + 1
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.size != self.m:
            raise ValueError(f"expected {self.m} labels, got {lab.size}")
        h = C.c_void_p()
        capi.check(self._lib.ellhip_svm_create(C.byref(h), self.m, self.nfeat, _p(data), _p(lab), int(device)),
                   "ellhip_svm_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ellhip_svm_destroy(h)

    # ---- OracleOptim
    def assess_optim(self, x, gamma: float):
        """((grad, SingleCut(beta)), shrunk, gamma): shrunk is always True; the incoming gamma is ignored"""
        x = _f64(x, self.n)
        g = np.empty(self.n, dtype=np.float64)
        b, sh, gm = C.c_double(), C.c_int(), C.c_double(gamma)
        capi.check(self._lib.ellhip_svm_assess_optim(self._h, _p(x), C.byref(gm), _p(g), C.byref(b), C.byref(sh)),
                   "ellhip_svm_assess_optim")
        return (g, SingleCut(b.value)), bool(sh.value), gm.value

    def margins(self, x) -> np.ndarray:
        """all m margins y_i * (w.x_i + b) at x"""
        x = _f64(x, self.n)
        out = np.empty(self.m, dtype=np.float64)
        capi.check(self._lib.ellhip_svm_margins(self._h, _p(x), _p(out)), "ellhip_svm_margins")
        return out

    def last(self):
        """(min_idx, min_val) of the last scan, as the reference leaves them"""
        i, v = C.c_int64(), C.c_double()
        capi.check(self._lib.ellhip_svm_last(self._h, C.byref(i), C.byref(v)), "ellhip_svm_last")
        return int(i.value), v.value

    # ---- device-resident driver loop
    def cutting_plane_optim(self, space, gamma: float, max_iters: int, tol: float):
        """(x_best or None, niter, gamma)"""
        xb = np.empty(self.n, dtype=np.float64)
        hb, ni, gm = C.c_int(), C.c_int64(), C.c_double(gamma)
        capi.check(self._lib.ellhip_svm_optim(space._h, self._h, C.byref(gm), int(max_iters), float(tol), _p(xb),
                                              C.byref(hb), C.byref(ni)), "ellhip_svm_optim")
        return (xb if hb.value else None), int(ni.value), gm.value
