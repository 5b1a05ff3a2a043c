"""Python mirror of the batched device-resident profit-maximisation loops (include/ellhip_batch_profit.h): B independent
`ProfitOracle`s, `ProfitRbOracle`s or `ProfitOracleQ`s (src/oracles/profit_oracle.rs), each with its own ellipsoid of
dimension 2; solved by one kernel per chunk of iterations on an `EllBatch` or an `EllStableBatch`.  The discrete kind runs
under `cutting_plane_optim_q`.  exp and ln are the library's own (csrc/ell_math.hpp), the same bits on host and device."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ell import _f64, _p

KINDS = {"plain": capi.PROFIT_PLAIN, "robust": capi.PROFIT_ROBUST, "discrete": capi.PROFIT_DISCRETE}


def math_eval(fn: str, x, device: int = -1):
    """ell_exp (fn = "exp") or ell_log ("log") of every element of x, on the device"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    capi.check(capi.load().ellhip_math_eval({"exp": 0, "log": 1}[fn], x.size, _p(x), _p(out), int(device)), "ellhip_math_eval")
    return out


class BatchProfitProblem:
    def __init__(self, kind, params, elasticities, price_out, vparams=None, *, device: int = -1):
        """kind: "plain", "robust" or "discrete" (or capi.PROFIT_*).  params [B][3] = (p, A, k), elasticities [B][2],
        price_out [B][2], vparams [B][5] for the robust kind."""
        self._lib = capi.load()
        kind = KINDS.get(kind, kind)
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 2 or params.shape[1] != 3:
            raise ValueError("params must be B x 3")
        B = params.shape[0]
        a = _f64(elasticities, 2 * B)
        v = _f64(price_out, 2 * B)
        vp = None if vparams is None else _f64(vparams, 5 * B)
        h = C.c_void_p()
        capi.check(self._lib.ellhip_batch_profit_create(C.byref(h), B, int(kind), _p(params), _p(a), _p(v), _p(vp), int(device)),
                   "ellhip_batch_profit_create")
        self._h = h
        self.B, self.n, self.kind = int(B), 2, int(kind)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ellhip_batch_profit_destroy(h)

    def set_chunk(self, iters: int):
        capi.check(self._lib.ellhip_batch_profit_set_chunk(self._h, int(iters)), "ellhip_batch_profit_set_chunk")

    def _gamma(self, gamma):
        return np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))

    def assess_optim(self, x, gamma):
        """One assess_optim per problem at x [B][2] with gamma [B] (or one value for all); the cursors advance.  Returns
        (grad [B][2], beta [B], shrunk [B] bool, gamma [B] afterwards)."""
        x = _f64(x, self.B * 2)
        gamma = self._gamma(gamma)
        grad = np.empty((self.B, 2))
        beta = np.empty(self.B)
        shrunk = np.empty(self.B, dtype=np.int32)
        capi.check(self._lib.ellhip_batch_profit_assess_optim(self._h, _p(x), _p(gamma), _p(grad), _p(beta), _p(shrunk)),
                   "ellhip_batch_profit_assess_optim")
        return grad, beta, shrunk.astype(bool), gamma

    def assess_optim_q(self, x, gamma, retry):
        """One assess_optim_q per problem with retry [B].  Returns
        (grad [B][2], beta [B], shrunk [B] bool, x_q [B][2], more_alt [B] bool, gamma [B] afterwards)."""
        x = _f64(x, self.B * 2)
        gamma = self._gamma(gamma)
        retry = np.ascontiguousarray(np.broadcast_to(np.asarray(retry), (self.B,)), dtype=np.int32)
        grad = np.empty((self.B, 2))
        x_q = np.empty((self.B, 2))
        beta = np.empty(self.B)
        shrunk = np.empty(self.B, dtype=np.int32)
        more = np.empty(self.B, dtype=np.int32)
        capi.check(self._lib.ellhip_batch_profit_assess_optim_q(self._h, _p(x), _p(gamma), _p(retry), _p(grad), _p(beta),
                                                                _p(shrunk), _p(x_q), _p(more)),
                   "ellhip_batch_profit_assess_optim_q")
        return grad, beta, shrunk.astype(bool), x_q, more.astype(bool), gamma

    def _loop(self, name, batch, gamma, max_iters, tol):
        gamma = self._gamma(gamma)
        entry = name + ("_stable" if batch.variant == capi.SPACE_ELL_STABLE else "")
        x_best, has, niter, status = capi.run_batch_loop(self._lib, entry, batch, self, gamma, max_iters, tol)
        return x_best, has, niter, gamma, status

    def optim(self, batch, gamma, max_iters: int, tol: float):
        """cutting_plane_optim per problem (plain and robust kinds) on `batch`, an EllBatch or an EllStableBatch of dimension
        2.  Returns (x_best [B][2] with NaN rows where there is none, has_best [B], niter [B], gamma [B], status [B])."""
        return self._loop("ellhip_batch_profit_optim", batch, gamma, max_iters, tol)

    def optim_q(self, batch, gamma, max_iters: int, tol: float):
        """cutting_plane_optim_q per problem (discrete kind); returns what `optim` returns, x_best being the oracle's x_q"""
        return self._loop("ellhip_batch_profit_optim_q", batch, gamma, max_iters, tol)
