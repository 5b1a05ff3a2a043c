"""Python mirror of the batched device-resident low-pass filter design loop (include/ellhip_batch_lowpass.h): B
independent `LowpassOracle`s (src/oracles/lowpass_oracle.rs) of one filter length n <= 128, each with its own band edges,
ripple limits and round-robin cursors and its own ellipsoid of an `EllBatch` or an `EllStableBatch`
(include/ellhip_batch_stable_loops.h), over one shared 15n x n table; solved by one kernel per chunk of iterations.
`BatchLowpassProblem.streamed` (include/ellhip_batch_lowpass_streamed.h) takes n up to 1024 and solves on an
`EllBatchStreamed` or an `EllStableBatchStreamed` (include/ellhip_batch_lowpass_streamed_stable.h).  Bit-identical to the
CPU arithmetic."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ell import _f64, _p

STATE_INTS = ("more_alt", "idx1", "idx2", "idx3", "kmax", "nwpass", "nwstop")
STATE_DOUBLES = ("fmax", "sp_sq")


# the entry point `name` of the engine and the variant of a batch handle (tests import it from here)
_loop_entry = capi.batch_loop_entry


class BatchLowpassProblem:
    def __init__(self, n: int, wpass, wstop, lp_sq, up_sq, sp_sq, spectrum=None, *, device: int = -1,
                 _create: str = "ellhip_batch_lowpass_create"):
        """wpass, wstop, lp_sq, up_sq, sp_sq: [B] each (scalars are broadcast to the longest); spectrum: the shared
        (15 n) x n table or None to have it computed as the reference does."""
        self._lib = capi.load()
        arrs = [np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (wpass, wstop, lp_sq, up_sq, sp_sq)]
        B = max(a.size for a in arrs)
        arrs = [np.ascontiguousarray(np.broadcast_to(a, (B,))) for a in arrs]
        n = int(n)
        spectrum = None if spectrum is None else _f64(spectrum, 15 * n * n)
        h = C.c_void_p()
        capi.check(getattr(self._lib, _create)(C.byref(h), B, n, *[_p(a) for a in arrs], _p(spectrum), device), _create)
        self._h = h
        self.B, self.n = int(B), n

    @classmethod
    def streamed(cls, n: int, wpass, wstop, lp_sq, up_sq, sp_sq, spectrum=None, *, device: int = -1):
        """The same problems for 1 <= n <= 1024 (include/ellhip_batch_lowpass_streamed.h): `optim` / `feas` then take an
        `EllBatchStreamed` or an `EllStableBatchStreamed`.  The table is kept twice in HBM, 2 * 15 n^2 * 8 bytes: 240 MiB at n = 1024."""
        return cls(n, wpass, wstop, lp_sq, up_sq, sp_sq, spectrum, device=device,
                   _create="ellhip_batch_lowpass_create_streamed")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ellhip_batch_lowpass_destroy(h)

    @property
    def spectrum(self):
        out = np.empty((15 * self.n, self.n))
        capi.check(self._lib.ellhip_batch_lowpass_get_spectrum(self._h, _p(out)), "ellhip_batch_lowpass_get_spectrum")
        return out

    def state(self):
        """dict of [B] arrays: more_alt, idx1, idx2, idx3, kmax, nwpass, nwstop (int32), fmax, sp_sq (float64)"""
        ints = np.empty((self.B, 7), dtype=np.int32)
        dbls = np.empty((self.B, 2))
        capi.check(self._lib.ellhip_batch_lowpass_state(self._h, _p(ints), _p(dbls)), "ellhip_batch_lowpass_state")
        out = {k: ints[:, j].copy() for j, k in enumerate(STATE_INTS)}
        out.update({k: dbls[:, j].copy() for j, k in enumerate(STATE_DOUBLES)})
        return out

    def reset(self):
        """cursors, fmax and kmax as after new()"""
        capi.check(self._lib.ellhip_batch_lowpass_reset(self._h), "ellhip_batch_lowpass_reset")

    def set_chunk(self, iters: int):
        capi.check(self._lib.ellhip_batch_lowpass_set_chunk(self._h, int(iters)), "ellhip_batch_lowpass_set_chunk")

    def assess_feas(self, x):
        """One assess_feas per problem.  Returns (grad [B][n], beta0 [B], has_beta1 [B], beta1 [B], cut [B]); rows of
        problems without a cut (cut[b] == 0) are NaN / 0."""
        x = _f64(x, self.B * self.n)
        grad = np.full((self.B, self.n), np.nan)
        beta0 = np.full(self.B, np.nan)
        beta1 = np.full(self.B, np.nan)
        has1 = np.zeros(self.B, dtype=np.int32)
        cut = np.empty(self.B, dtype=np.int32)
        capi.check(self._lib.ellhip_batch_lowpass_assess_feas(self._h, _p(x), _p(grad), _p(beta0), _p(has1), _p(beta1),
                                                              _p(cut)), "ellhip_batch_lowpass_assess_feas")
        return grad, beta0, has1, beta1, cut

    def assess_optim(self, x, gamma):
        """One assess_optim per problem.  Returns (grad, beta0, has_beta1, beta1, shrunk [B], gamma [B], rc [B]); rc[b] is
        1, or capi.E_STATE where the reference would panic (that problem's rows are NaN / 0, its gamma unchanged)."""
        x = _f64(x, self.B * self.n)
        gamma = np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))
        grad = np.full((self.B, self.n), np.nan)
        beta0 = np.full(self.B, np.nan)
        beta1 = np.full(self.B, np.nan)
        has1 = np.zeros(self.B, dtype=np.int32)
        shrunk = np.empty(self.B, dtype=np.int32)
        rc = np.empty(self.B, dtype=np.int32)
        capi.check(self._lib.ellhip_batch_lowpass_assess_optim(self._h, _p(x), _p(gamma), _p(grad), _p(beta0), _p(has1),
                                                               _p(beta1), _p(shrunk), _p(rc)),
                   "ellhip_batch_lowpass_assess_optim")
        return grad, beta0, has1, beta1, shrunk, gamma, rc

    def optim(self, batch, gamma, max_iters: int, tol: float):
        """cutting_plane_optim per problem on `batch` (an EllBatch, an EllStableBatch, an EllBatchStreamed or an
        EllStableBatchStreamed).  Returns
        (x_best [B][n] with NaN rows where there is none, has_best [B], niter [B], gamma [B], status [B])."""
        gamma = np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))
        x_best, has, niter, status = capi.run_batch_loop(self._lib, _loop_entry(batch, "ellhip_batch_lowpass_optim"), batch,
                                                         self, gamma, max_iters, tol)
        return x_best, has, niter, gamma, status

    def feas(self, batch, max_iters: int, tol: float):
        """cutting_plane_feas per problem.  Returns (x [B][n] with NaN rows where none was found, feasible [B], niter [B],
        status [B])."""
        return capi.run_batch_loop(self._lib, _loop_entry(batch, "ellhip_batch_lowpass_feas"), batch, self, None, max_iters,
                                   tol)
