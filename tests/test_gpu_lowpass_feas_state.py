"""GPU: ellhip_lowpass_feas leaves the search space where the host-driven cutting_plane_feas leaves it, Q included.  On Ell
at depth 1 the shrink of a cut rides on the next iteration's commit; when the oracle ends the loop feasible at the top of
that iteration, the driver has to apply it afterwards (csrc/device_loop.inc.hpp)."""
import numpy as np
import pytest

from lowpass_probes import CONSTANT_SETS

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def host_feas(o, space, max_iters, tol):
    """cutting_plane_feas (src/cutting_plane.rs:205-227) with the device oracle behind assess_feas and ellhip_update"""
    for niter in range(max_iters):
        x = space.xc()
        cut = o.assess_feas(x)
        if cut is None:
            return x, niter
        if int(space.update_bias_cut(cut)) != 0 or space.tsq() < tol:
            return None, niter
    return None, max_iters


@pytest.mark.parametrize("variant,depth", [("ell", 1), ("ell", 8), ("stable", None)])
def test_feasible_end_leaves_the_host_loops_space(gpu, variant, depth):
    n = 32
    c = CONSTANT_SETS["loose"]

    def space():
        if variant == "stable":
            return gpu.EllStable.new_with_scalar(40.0, np.zeros(n))
        s = gpu.Ell.new_with_scalar(40.0, np.zeros(n))
        s.defer_depth = depth
        return s

    sh, sd = space(), space()
    x_h, ni_h = host_feas(gpu.LowpassOracle(n, *c), sh, 2000, 1e-14)
    x_d, ni_d = gpu.LowpassOracle(n, *c).cutting_plane_feas(sd, 2000, 1e-14)
    if variant == "ell":   # ends feasible, behind at least one cut whose shrink is still pending at depth 1
        assert x_h is not None and ni_h > 3
    # (on EllStable this problem ends without a point, tests/test_gpu_lowpass.py::test_feas_loop: the same comparisons hold)
    assert ni_d == ni_h and (x_d is None) == (x_h is None) and (x_h is None or same_bits(x_d, x_h))
    assert same_bits(sd.xc(), sh.xc()) and same_bits(sd.kappa, sh.kappa) and same_bits(sd.tsq(), sh.tsq())
    assert same_bits(sd.mq, sh.mq)
