"""CPU reference of the batched LMI cutting-plane loop (include/ellhip_batch_lmi.h): the J-block round-robin oracle of
tests/lmi_tests.rs:142-171 restated over oracle.OracleLMI, cutting_plane_optim / cutting_plane_feas
(src/cutting_plane.rs:286-313, 205-227) over oracle.OracleEll, and the generators of the test families."""
import math

import numpy as np

from oracle import oracle as O

# tests/lmi_tests.rs:14-52
F1 = np.array([[[-7.0, -11.0], [-11.0, 3.0]], [[7.0, -18.0], [-18.0, 8.0]], [[-2.0, -8.0], [-8.0, 1.0]]])
B1 = np.array([[33.0, -9.0], [-9.0, 26.0]])
F2 = np.array([[[-21.0, -11.0, 0.0], [-11.0, 10.0, 8.0], [0.0, 8.0, 5.0]],
               [[0.0, 10.0, 16.0], [10.0, -10.0, -10.0], [16.0, -10.0, 3.0]],
               [[-5.0, 2.0, -17.0], [2.0, -6.0, 8.0], [-17.0, 8.0, 6.0]]])
B2 = np.array([[14.0, 9.0, 40.0], [9.0, 91.0, 10.0], [40.0, 10.0, 15.0]])
C_REF = np.array([1.0, -1.0, 1.0])

SUCCESS, NOSOLN = 0, 1


class RoundRobinLmi:
    """mat_f: J arrays [n][m_j][m_j]; mat_b: J arrays [m_j][m_j] or None (LMI0 form); c: [n] or None (stations are the
    J blocks only)."""

    def __init__(self, mat_f, mat_b=None, c=None):
        self.J = len(mat_f)
        self.idx = -1
        self.c = None if c is None else np.array(c, dtype=np.float64)
        self.blocks = [O.OracleLMI(f, None if mat_b is None else mat_b[j]) for j, f in enumerate(mat_f)]

    def assess_optim(self, xc, gamma):
        """-> (g, beta), station, gamma; station J = objective cut, J + 1 = shrunk"""
        J = self.J
        f0 = 0.0
        for a, b in zip(self.c.tolist(), np.asarray(xc).tolist()):
            f0 += a * b
        for _ in range(J + 1):
            self.idx = 0 if self.idx >= J else self.idx + 1
            if self.idx < J:
                cut = self.blocks[self.idx].assess_feas(xc)
                if cut is not None:
                    return (cut[0], cut[1]), self.idx, gamma
            else:
                fj = f0 - gamma
                if fj > 0.0:
                    return (self.c.copy(), fj), J, gamma
                gamma = f0
        return (self.c.copy(), 0.0), J + 1, gamma

    def assess_feas(self, xc):
        """-> (g, beta), station, or None when every block passes"""
        for _ in range(self.J):
            self.idx = 0 if self.idx >= self.J - 1 else self.idx + 1
            cut = self.blocks[self.idx].assess_feas(xc)
            if cut is not None:
                return (cut[0], cut[1]), self.idx
        return None


def optim(space, omega, gamma, max_iters, tol):
    """cutting_plane_optim -> (x_best or None, niter, gamma, status of the last update)"""
    x_best, status = None, SUCCESS
    for niter in range(max_iters):
        x = np.array(space.xc)
        (g, beta), station, gamma = omega.assess_optim(x, gamma)
        if station == omega.J + 1:
            x_best = x
            status = space.update_central_cut(g, beta)
        else:
            status = space.update_bias_cut(g, beta)
        if status != SUCCESS or space.tsq < tol:
            return x_best, niter, gamma, status
    return x_best, max_iters, gamma, SUCCESS


def feas(space, omega, max_iters, tol):
    """cutting_plane_feas -> (x or None, niter, status of the last update; Success when feasible)"""
    for niter in range(max_iters):
        x = np.array(space.xc)
        cut = omega.assess_feas(x)
        if cut is None:
            return x, niter, SUCCESS
        (g, beta), _ = cut
        status = space.update_bias_cut(g, beta)
        if status != SUCCESS or space.tsq < tol:
            return None, niter, status
    return None, max_iters, SUCCESS


def sym(a):
    return (a + np.swapaxes(a, -1, -2)) / 2


def reference_problem():
    return [F1.copy(), F2.copy()], [B1.copy(), B2.copy()], C_REF.copy()


def family_a(seed, e=0.05):
    """the perturbed reference problem"""
    rng = np.random.default_rng(1000 + seed)
    f1 = F1 + e * sym(rng.standard_normal(F1.shape))
    b1 = B1 + e * sym(rng.standard_normal(B1.shape))
    f2 = F2 + e * sym(rng.standard_normal(F2.shape))
    b2 = B2 + e * sym(rng.standard_normal(B2.shape))
    c = C_REF + e * rng.standard_normal(3)
    return [f1, f2], [b1, b2], c


def family_b(seed, n, m, J):
    """random strictly feasible pencils (x = 0 is strictly feasible: B_j > 0)"""
    rng = np.random.default_rng(7000 + seed)
    fs = [sym(rng.standard_normal((n, m, m))) for _ in range(J)]
    bs = []
    for _ in range(J):
        mm = rng.standard_normal((m, m))
        bs.append(mm @ mm.T + m * np.eye(m))
    c = rng.standard_normal(n)
    return fs, bs, c


def stack(problems):
    """[(fs, bs, c)] per instance -> (mat_f: J arrays [B][n][m][m], mat_b: J arrays [B][m][m], c [B][n])"""
    J = len(problems[0][0])
    mat_f = [np.stack([p[0][j] for p in problems]) for j in range(J)]
    mat_b = [np.stack([p[1][j] for p in problems]) for j in range(J)]
    return mat_f, mat_b, np.stack([p[2] for p in problems])


def new_space(n, kappa=10.0):
    return O.OracleEll.new_with_scalar(kappa, np.zeros(n))


def run_optim(problems, max_iters, tol, *, lmi0=False, gamma=math.inf):
    """every instance on a fresh Ell::new_with_scalar(10, 0) -> list of dicts, plus the spaces and oracles"""
    out, spaces, omegas = [], [], []
    for fs, bs, c in problems:
        space = new_space(len(c))
        omega = RoundRobinLmi(fs, None if lmi0 else bs, c)
        x_best, niter, g, status = optim(space, omega, gamma, max_iters, tol)
        out.append(dict(x_best=x_best, niter=niter, gamma=g, status=status, idx=omega.idx))
        spaces.append(space)
        omegas.append(omega)
    return out, spaces, omegas
