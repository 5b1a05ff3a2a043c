"""Python mirror of the batched device-resident max-cut cutting-plane loops (include/ellhip_batch_maxcut.h): B independent
`MaxcutOracle`s (src/oracles/maxcut_oracle.rs) of one size n <= 1024, each with its own ellipsoid of dimension n, over one
shared weight table or one table per problem; solved by one kernel per chunk of iterations on an `EllBatch` or an
`EllStableBatch` (n <= 128), an `EllBatchStreamed` or an `EllStableBatchStreamed`.  Bit-identical to the CPU arithmetic."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ell import _f64, _p


class BatchMaxcutProblem:
    def __init__(self, weights, B: int | None = None, *, shared=None, device: int = -1):
        """weights: n x n (one table for every problem; B says how many there are) or B x n x n.  shared: None = inferred
        from weights.ndim."""
        self._lib = capi.load()
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if shared is None:
            shared = w.ndim == 2
        if w.ndim != (2 if shared else 3) or w.shape[-1] != w.shape[-2]:
            raise ValueError("weights must be n x n (shared) or B x n x n")
        if shared:
            if B is None:
                raise ValueError("a shared table needs B")
        elif B is None:
            B = w.shape[0]
        elif B != w.shape[0]:
            raise ValueError(f"weights has shape {w.shape}, B is {B}")
        n = w.shape[-1]
        h = C.c_void_p()
        capi.check(self._lib.ellhip_batch_maxcut_create(C.byref(h), int(B), n, _p(w), int(bool(shared)), int(device)),
                   "ellhip_batch_maxcut_create")
        self._h = h
        self.B, self.n, self.shared = int(B), int(n), bool(shared)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ellhip_batch_maxcut_destroy(h)

    def set_chunk(self, iters: int):
        capi.check(self._lib.ellhip_batch_maxcut_set_chunk(self._h, int(iters)), "ellhip_batch_maxcut_set_chunk")

    def assess_optim(self, x, gamma):
        """One assess_optim per problem at x [B][n] with gamma [B] (or one value for all).  Returns
        (grad [B][n], beta [B], shrunk [B] bool, gamma [B] afterwards, cut_value [B])."""
        x = _f64(x, self.B * self.n)
        gamma = np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))
        grad = np.empty((self.B, self.n))
        beta = np.empty(self.B)
        cut = np.empty(self.B)
        shrunk = np.empty(self.B, dtype=np.int32)
        capi.check(self._lib.ellhip_batch_maxcut_assess_optim(self._h, _p(x), _p(gamma), _p(grad), _p(beta), _p(shrunk),
                                                              _p(cut)), "ellhip_batch_maxcut_assess_optim")
        return grad, beta, shrunk.astype(bool), gamma, cut

    def optim(self, batch, gamma, max_iters: int, tol: float):
        """cutting_plane_optim per problem on `batch` (an EllBatch, an EllStableBatch, an EllBatchStreamed or an
        EllStableBatchStreamed of dimension n).  Returns
        (x_best [B][n] with NaN rows where there is none, has_best [B], niter [B], gamma [B], status [B])."""
        gamma = np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))
        entry = capi.batch_loop_entry(batch, "ellhip_batch_maxcut_optim")
        x_best, has, niter, status = capi.run_batch_loop(self._lib, entry, batch, self, gamma, max_iters, tol)
        return x_best, has, niter, gamma, status
