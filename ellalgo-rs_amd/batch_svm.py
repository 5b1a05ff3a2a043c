"""Python mirror of the batched device-resident SVM cutting-plane loop (include/ellhip_batch_svm.h): B independent
`SvmOracle`s (src/oracles/svm_oracle.rs) of one shape (m samples, nfeat <= 127 features), each with its own labels and its
own ellipsoid of an `EllBatch` (dimension nfeat + 1), over one shared table or one table per problem; solved by one kernel
per chunk of iterations.  `BatchSvmProblem.streamed` (include/ellhip_batch_svm_streamed.h) takes nfeat up to 1023 and solves
on an `EllBatchStreamed` or an `EllStableBatchStreamed`.  Bit-identical to the CPU arithmetic."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ell import _f64, _p


# the entry point `name` of the engine and the variant of a batch handle (tests import it from here)
_loop_entry = capi.batch_loop_entry


class BatchSvmProblem:
    def __init__(self, data, labels, *, shared=None, device: int = -1, _create: str = "ellhip_batch_svm_create"):
        """data: m x nfeat (one table for every problem) or B x m x nfeat; labels: B x m integers (stored as int32,
        converted `as f64`).  shared: None = inferred from data.ndim."""
        self._lib = capi.load()
        data = np.ascontiguousarray(data, dtype=np.float64)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if shared is None:
            shared = data.ndim == 2
        if lab.ndim != 2 or data.ndim != (2 if shared else 3):
            raise ValueError("labels must be B x m and data m x nfeat (shared) or B x m x nfeat")
        B, m = lab.shape
        nfeat = data.shape[-1]
        if data.shape[:-1] != ((m,) if shared else (B, m)):
            raise ValueError(f"data has shape {data.shape}, labels {lab.shape}")
        h = C.c_void_p()
        capi.check(getattr(self._lib, _create)(C.byref(h), B, m, nfeat, _p(data), int(bool(shared)), _p(lab), int(device)),
                   _create)
        self._h = h
        self.B, self.m, self.nfeat, self.n, self.shared = int(B), int(m), int(nfeat), int(nfeat) + 1, bool(shared)

    @classmethod
    def streamed(cls, data, labels, *, shared=None, device: int = -1):
        """The same problems for 1 <= nfeat <= 1023 (include/ellhip_batch_svm_streamed.h): `optim` then takes an
        `EllBatchStreamed` or an `EllStableBatchStreamed` of dimension nfeat + 1."""
        return cls(data, labels, shared=shared, device=device, _create="ellhip_batch_svm_create_streamed")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ellhip_batch_svm_destroy(h)

    def set_chunk(self, iters: int):
        capi.check(self._lib.ellhip_batch_svm_set_chunk(self._h, int(iters)), "ellhip_batch_svm_set_chunk")

    def margins(self, x):
        """all margins at x [B][n]: [B][m]"""
        x = _f64(x, self.B * self.n)
        out = np.empty((self.B, self.m))
        capi.check(self._lib.ellhip_batch_svm_margins(self._h, _p(x), _p(out)), "ellhip_batch_svm_margins")
        return out

    def assess_optim(self, x):
        """One assess_optim per problem at x [B][n].  Returns (grad [B][n], beta [B], gamma [B]); `shrunk` is always
        true."""
        x = _f64(x, self.B * self.n)
        grad = np.empty((self.B, self.n))
        beta = np.empty(self.B)
        gamma = np.empty(self.B)
        capi.check(self._lib.ellhip_batch_svm_assess_optim(self._h, _p(x), _p(gamma), _p(grad), _p(beta)),
                   "ellhip_batch_svm_assess_optim")
        return grad, beta, gamma

    def last(self):
        """(min_idx [B] int64, min_val [B]) of each problem's last scan; 0 and +inf when no margin was below +inf"""
        idx = np.empty(self.B, dtype=np.int64)
        val = np.empty(self.B)
        capi.check(self._lib.ellhip_batch_svm_last(self._h, _p(idx), _p(val)), "ellhip_batch_svm_last")
        return idx, val

    def optim(self, batch, gamma, max_iters: int, tol: float):
        """cutting_plane_optim per problem on `batch` (an EllBatch, an EllStableBatch, an EllBatchStreamed or an
        EllStableBatchStreamed of dimension nfeat + 1).  Returns
        (x_best [B][n] with NaN rows where there is none, has_best [B], niter [B], gamma [B], status [B])."""
        gamma = np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))
        x_best, has, niter, status = capi.run_batch_loop(self._lib, _loop_entry(batch, "ellhip_batch_svm_optim"), batch, self,
                                                         gamma, max_iters, tol)
        return x_best, has, niter, gamma, status
