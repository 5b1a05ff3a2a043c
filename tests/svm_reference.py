"""Restatement of the reference's `SvmOracle` (src/oracles/svm_oracle.rs:4-58) and of `cutting_plane_optim`
(src/cutting_plane.rs:286-313) in numpy, for the SVM tests.  Test infrastructure, not product code.

Margins fold the products left to right from -0.0 (Arr::dot: `.map(|(a, b)| a * b).sum()`, src/arr.rs:443-451),
vectorised over the samples; np.sum / @ use other orders and are not used.  The argmin is a literal loop."""
import numpy as np


def margins(data, labels, x):
    data = np.asarray(data, dtype=np.float64)
    nfeat = data.shape[1]
    x = np.asarray(x, dtype=np.float64)
    acc = np.full(data.shape[0], -0.0)
    with np.errstate(invalid="ignore", over="ignore"):   # 0 * inf and inf - inf are NaN, as in the reference
        for j in range(nfeat):
            acc = acc + x[j] * data[:, j]
        return np.asarray(labels, dtype=np.int32).astype(np.float64) * (acc + x[nfeat])


def argmin(mg):
    """(min_idx, min_val): min_val starts at +inf, min_idx at 0, replaced only when margin < min_val"""
    min_val, min_idx = np.inf, 0
    for i, v in enumerate(mg.tolist()):
        if v < min_val:
            min_val, min_idx = v, i
    return min_idx, min_val


def assess_optim(data, labels, x):
    """((grad, beta), shrunk, gamma, min_idx, min_val) exactly as the reference computes them"""
    data = np.asarray(data, dtype=np.float64)
    nfeat = data.shape[1]
    idx, val = argmin(margins(data, labels, x))
    if val >= 1.0:
        return (np.zeros(nfeat + 1), 0.0), True, 0.0, idx, val
    y = float(np.int32(labels[idx]))
    g = np.append((-y) * data[idx], -y)
    return (g, val), True, val, idx, val


def cutting_plane_optim(data, labels, space, gamma, max_iters, tol):
    """the reference loop over an oracle OracleEll / OracleEllStable: (x_best, niter, gamma, chosen indices)"""
    x_best, chosen = None, []
    for niter in range(max_iters):
        (g, beta), shrunk, gamma, idx, _ = assess_optim(data, labels, np.array(space.xc))
        chosen.append(idx)
        x_best = np.array(space.xc)   # shrunk is always true
        status = space.update_central_cut(g, beta)
        if status != 0 or space.tsq < tol:
            return x_best, niter, gamma, chosen
    return x_best, max_iters, gamma, chosen
