"""Python mirror of the batched device-resident LMI cutting-plane loop (include/ellhip_batch_lmi.h): B independent
problems `min c'x  s.t.  B_j - sum_k x_k F_jk > 0` (or, without mat_b, `sum_k x_k F_jk > 0`), each with its own
round-robin oracle (tests/lmi_tests.rs:142-171 generalised to J blocks) and its own ellipsoid of an `EllBatch` or an
`EllStableBatch` (include/ellhip_batch_stable_loops.h), solved by one kernel per chunk of iterations.
`BatchLmiProblem.streamed` (include/ellhip_batch_lmi_streamed.h) takes n up to 1024, with one pencil per problem or one for
all of them, and solves on an `EllBatchStreamed` or an `EllStableBatchStreamed`.  Bit-identical to the CPU arithmetic."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ell import _f64, _p


# the entry point `name` of the engine and the variant of a batch handle (tests import it from here)
_loop_entry = capi.batch_loop_entry


class BatchLmiProblem:
    def __init__(self, mat_f, mat_b=None, c=None, *, device: int = -1, _streamed: bool = False, _shared: bool = False):
        """mat_f: a list of J arrays [B][n][m_j][m_j]; mat_b: a list of J arrays [B][m_j][m_j] or None (LMI0 form);
        c: [B][n] or None (feasibility problem)."""
        self._lib = capi.load()
        mat_f = [np.ascontiguousarray(f, dtype=np.float64) for f in mat_f]
        if _shared:
            if not mat_f or any(f.ndim != 3 or f.shape[1] != f.shape[2] for f in mat_f):
                raise ValueError("a shared mat_f must be a list of [n][m][m] arrays")
            if mat_b is None and c is None:
                raise ValueError("a shared pencil needs mat_b or c to tell the number of problems")
            B = len(mat_b[0]) if mat_b is not None else np.asarray(c).shape[0]
            mat_f = [f[None] for f in mat_f]
        elif not mat_f or any(f.ndim != 4 or f.shape[2] != f.shape[3] for f in mat_f):
            raise ValueError("mat_f must be a list of [B][n][m][m] arrays")
        else:
            B = mat_f[0].shape[0]
        n = mat_f[0].shape[1]
        if any(f.shape[:2] != (1 if _shared else B, n) for f in mat_f):
            raise ValueError("every block needs the same B and n")
        m = np.array([f.shape[2] for f in mat_f], dtype=np.int64)
        flat_f = np.concatenate([f.ravel() for f in mat_f])
        flat_b = None
        if mat_b is not None:
            mat_b = [np.ascontiguousarray(b, dtype=np.float64) for b in mat_b]
            if len(mat_b) != len(mat_f) or any(b.shape != (B, mj, mj) for b, mj in zip(mat_b, m)):
                raise ValueError("mat_b must be a list of [B][m][m] arrays, one per block")
            flat_b = np.concatenate([b.ravel() for b in mat_b])
        c = None if c is None else _f64(c, B * n)
        h = C.c_void_p()
        if _streamed:
            capi.check(self._lib.ellhip_batch_lmi_create_streamed(C.byref(h), B, n, len(mat_f), _p(m), _p(flat_f),
                                                                  int(bool(_shared)), _p(flat_b), _p(c), device),
                       "ellhip_batch_lmi_create_streamed")
        else:
            capi.check(self._lib.ellhip_batch_lmi_create(C.byref(h), B, n, len(mat_f), _p(m), _p(flat_f), _p(flat_b), _p(c),
                                                         device), "ellhip_batch_lmi_create")
        self._h = h
        self.B, self.n, self.J = int(B), int(n), len(mat_f)
        self.has_c = c is not None
        self.shared = bool(_shared)

    @classmethod
    def streamed(cls, mat_f, mat_b=None, c=None, *, shared: bool = False, device: int = -1):
        """The same problems for 1 <= n <= 1024 (include/ellhip_batch_lmi_streamed.h): `optim` / `feas` then take an
        `EllBatchStreamed` or an `EllStableBatchStreamed`.  shared: mat_f is a list of J arrays [n][m_j][m_j], one pencil
        that every problem reads; mat_b and c stay per problem (one of them must be given: it tells B)."""
        return cls(mat_f, mat_b, c, device=device, _streamed=True, _shared=shared)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ellhip_batch_lmi_destroy(h)

    @property
    def idx(self):
        out = np.empty(self.B, dtype=np.int32)
        capi.check(self._lib.ellhip_batch_lmi_get_idx(self._h, _p(out)), "ellhip_batch_lmi_get_idx")
        return out

    @idx.setter
    def idx(self, value):
        v = None if value is None else np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.int32), (self.B,)))
        capi.check(self._lib.ellhip_batch_lmi_set_idx(self._h, _p(v)), "ellhip_batch_lmi_set_idx")

    def set_chunk(self, iters: int):
        capi.check(self._lib.ellhip_batch_lmi_set_chunk(self._h, int(iters)), "ellhip_batch_lmi_set_chunk")

    def assess_optim(self, x, gamma):
        """One oracle call per problem.  Returns (grad [B][n], beta [B], station [B], gamma [B]); station J = objective
        cut, J + 1 = shrunk."""
        x = _f64(x, self.B * self.n)
        gamma = np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))
        grad = np.zeros((self.B, self.n))
        beta = np.empty(self.B)
        station = np.empty(self.B, dtype=np.int32)
        capi.check(self._lib.ellhip_batch_lmi_assess_optim(self._h, _p(x), _p(gamma), _p(grad), _p(beta), _p(station)),
                   "ellhip_batch_lmi_assess_optim")
        return grad, beta, station, gamma

    def optim(self, spaces, gamma, max_iters: int, tol: float):
        """cutting_plane_optim per problem on `spaces` (an EllBatch, an EllStableBatch, an EllBatchStreamed or an
        EllStableBatchStreamed).  Returns (x_best [B][n] with NaN rows where there
        is none, has_best [B], niter [B], gamma [B], status [B])."""
        gamma = np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))
        x_best, has, niter, status = capi.run_batch_loop(self._lib, _loop_entry(spaces, "ellhip_batch_lmi_optim"), spaces, self,
                                                         gamma, max_iters, tol)
        return x_best, has, niter, gamma, status

    def feas(self, spaces, max_iters: int, tol: float):
        """cutting_plane_feas per problem.  Returns (x [B][n] with NaN rows where infeasible, feasible [B], niter [B],
        status [B])."""
        return capi.run_batch_loop(self._lib, _loop_entry(spaces, "ellhip_batch_lmi_feas"), spaces, self, None, max_iters, tol)
