"""Python mirror of the batched linear feasibility oracles with a movable target and of the batched device-resident bsearch
over them (include/ellhip_batch_bsearch.h): B `MyOracle3`-like oracles (src/example3.rs) of J rows in n variables, each
with its own ellipsoid in an `EllBatch` or an `EllStableBatch`; `bsearch` runs the reference's `bsearch` over
`BSearchAdaptor` (src/cutting_plane.rs:403-419, :441-466) for all of them in one kernel per chunk of rounds.
`BatchLinFeasProblem.streamed` (include/ellhip_batch_bsearch_streamed.h) takes n up to 1024 and J up to 4096 and runs on an
`EllBatchStreamed` or an `EllStableBatchStreamed`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ell import _f64, _p

# every symbol include/ellhip_batch_bsearch.h declares, with its prototype (kept here, apart from capi.EXPORTS)
_vp, _i32, _i64, _dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_FEAS = (_i32, [_vp, _vp, _i64, _dbl, _vp, _vp, _vp, _vp])
_BSEARCH = (_i32, [_vp, _vp, _vp, _vp, _i64, _dbl, _i64, _dbl, _vp, _vp, _vp, _vp, _vp])
PROTOTYPES = {
    "ellhip_batch_linfeas_create": (_i32, [C.POINTER(_vp), _i64, _i64, _i64, _vp, _vp, _i32, _i32]),
    "ellhip_batch_linfeas_destroy": (None, [_vp]),
    "ellhip_batch_linfeas_set_chunk": (_i32, [_vp, _i64]),
    "ellhip_batch_linfeas_set_target": (_i32, [_vp, _vp]),
    "ellhip_batch_linfeas_state": (_i32, [_vp, _vp, _vp]),
    "ellhip_batch_linfeas_assess_feas": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "ellhip_batch_linfeas_feas": _FEAS,
    "ellhip_batch_linfeas_feas_stable": _FEAS,
    "ellhip_batch_linfeas_bsearch": _BSEARCH,
    "ellhip_batch_linfeas_bsearch_stable": _BSEARCH,
}
BATCH_BSEARCH_NAMES = sorted(PROTOTYPES)
# every symbol include/ellhip_batch_bsearch_streamed.h declares (each as its counterpart above)
STREAMED_PROTOTYPES = {
    "ellhip_batch_linfeas_create_streamed": PROTOTYPES["ellhip_batch_linfeas_create"],
    "ellhip_batch_linfeas_feas_streamed": _FEAS,
    "ellhip_batch_linfeas_feas_streamed_stable": _FEAS,
    "ellhip_batch_linfeas_bsearch_streamed": _BSEARCH,
    "ellhip_batch_linfeas_bsearch_streamed_stable": _BSEARCH,
}
BATCH_BSEARCH_STREAMED_NAMES = sorted(STREAMED_PROTOTYPES)


def _load():
    lib = capi.load()
    if getattr(lib.ellhip_batch_linfeas_create, "argtypes", None) is None:
        for name, (res, args) in {**PROTOTYPES, **STREAMED_PROTOTYPES}.items():
            fn = getattr(lib, name)  # a missing symbol is an error
            fn.restype, fn.argtypes = res, args
    return lib


class BatchLinFeasProblem:
    def __init__(self, a, c, B: int | None = None, *, device: int = -1, _create: str = "ellhip_batch_linfeas_create"):
        """a [J][n] and c [J] with B: one table for all B problems; a [B][J][n] and c [B][J]: a table per problem.  The last
        entry of every c is never read (the last row's offset is the target)."""
        self._lib = _load()
        self._by_handle = _create != "ellhip_batch_linfeas_create"  # made by `streamed`: the batch handle picks the engine
        a = np.ascontiguousarray(a, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        if a.ndim == 2:
            if B is None:
                raise ValueError("a shared table needs B")
            shared, (J, n) = 1, a.shape
            if c.shape != (J,):
                raise ValueError("c must be [J]")
        elif a.ndim == 3:
            shared, (Ba, J, n) = 0, a.shape
            if B is not None and int(B) != Ba:
                raise ValueError("B differs from a's first dimension")
            B = Ba
            if c.shape != (B, J):
                raise ValueError("c must be [B][J]")
        else:
            raise ValueError("a must be [J][n] or [B][J][n]")
        h = C.c_void_p()
        capi.check(getattr(self._lib, _create)(C.byref(h), int(B), n, J, _p(a), _p(c), shared, int(device)), _create)
        self._h = h
        self.B, self.n, self.J = int(B), int(n), int(J)

    @classmethod
    def streamed(cls, a, c, B: int | None = None, *, device: int = -1):
        """The same problems for 1 <= n <= 1024 and 1 <= J <= 4096 (include/ellhip_batch_bsearch_streamed.h): `feas` and
        `bsearch` then run on the engine of the batch handle they are given, an `EllBatchStreamed` or an
        `EllStableBatchStreamed` of dimension n among them."""
        return cls(a, c, B, device=device, _create="ellhip_batch_linfeas_create_streamed")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ellhip_batch_linfeas_destroy(h)

    def set_chunk(self, iters: int):
        capi.check(self._lib.ellhip_batch_linfeas_set_chunk(self._h, int(iters)), "ellhip_batch_linfeas_set_chunk")

    def _vec(self, v):
        return np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.B,)))

    def set_target(self, gamma):
        """update(gamma) per problem (gamma [B] or one value for all)"""
        gamma = self._vec(gamma)
        capi.check(self._lib.ellhip_batch_linfeas_set_target(self._h, _p(gamma)), "ellhip_batch_linfeas_set_target")

    def state(self):
        """(idx [B] int32, target [B])"""
        idx = np.empty(self.B, dtype=np.int32)
        target = np.empty(self.B)
        capi.check(self._lib.ellhip_batch_linfeas_state(self._h, _p(idx), _p(target)), "ellhip_batch_linfeas_state")
        return idx, target

    def assess_feas(self, x):
        """One assess_feas per problem at x [B][n]; the cursors advance.  Returns (grad [B][n], beta [B], cut [B]): cut[b] is
        the row that answered or -1 for None."""
        x = _f64(x, self.B * self.n)
        grad = np.empty((self.B, self.n))
        beta = np.empty(self.B)
        cut = np.empty(self.B, dtype=np.int32)
        capi.check(self._lib.ellhip_batch_linfeas_assess_feas(self._h, _p(x), _p(grad), _p(beta), _p(cut)),
                   "ellhip_batch_linfeas_assess_feas")
        return grad, beta, cut

    def _entry(self, batch, name):
        if self._by_handle:
            return capi.batch_loop_entry(batch, name)
        # (the plain constructor's dispatch: a streamed handle goes to the LDS entry points, which refuse it)
        return name + ("_stable" if batch.variant == capi.SPACE_ELL_STABLE else "")

    def feas(self, batch, max_iters: int, tol: float):
        """cutting_plane_feas per problem on `batch` (an EllBatch or an EllStableBatch; a streamed one for `streamed`).
        Returns (x [B][n] with NaN rows where none is feasible, feasible [B], niter [B], status [B])."""
        entry = self._entry(batch, "ellhip_batch_linfeas_feas")
        return capi.run_batch_loop(self._lib, entry, batch, self, None, max_iters, tol)

    def bsearch(self, batch, lower, upper, inner_max_iters: int, inner_tol: float, max_iters: int, tol: float):
        """bsearch over BSearchAdaptor per problem; `batch` is the adaptor's space.  Returns (feasible [B] bool, niter [B],
        upper [B], rounds [B], ends [B][4])."""
        entry = self._entry(batch, "ellhip_batch_linfeas_bsearch")
        lower, upper = self._vec(lower), self._vec(upper)
        feasible = np.empty(self.B, dtype=np.int32)
        niter = np.empty(self.B, dtype=np.int64)
        upper_out = np.empty(self.B)
        rounds = np.empty(self.B, dtype=np.int64)
        ends = np.empty((self.B, 4), dtype=np.int64)
        capi.check(getattr(self._lib, entry)(batch._h, self._h, _p(lower), _p(upper), int(inner_max_iters), float(inner_tol),
                                             int(max_iters), float(tol), _p(feasible), _p(niter), _p(upper_out), _p(rounds),
                                             _p(ends)), entry)
        return feasible.astype(bool), niter, upper_out, rounds, ends
