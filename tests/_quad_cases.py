"""The problems and the parity bar that the CDQuadraticLoss tests share (test_gpu_quad.py, test_gpu_quad_batch.py).

A = X'X / n of a Gaussian X with n = 2p + 2 rows: positive diagonal, well conditioned.  The bar, against
the oracle's per-coordinate sweep of the same problem: beta within 1e-10, the SAME passes, full passes, visits and convergence
flag, and the same support ORDER (nzval2ind)."""
import functools

import numpy as np

BETA_TOL = 1e-10
H_TOL = 1e-12                           # the signed h of a visit, max |h| of a pass
OPT = dict(maxIter=20000, optTol=1e-12)


@functools.lru_cache(maxsize=None)
def _A(p, seed=0):
    rng = np.random.default_rng(1000 * seed + p)
    X = rng.standard_normal((2 * p + 2, p))
    A = X.T @ X / X.shape[0]
    A = (A + A.T) / 2
    A.setflags(write=False)
    return A


def _b(p, seed, s=None):
    """b = -(A beta* + noise): the covariance form of a regression on s planted coordinates."""
    rng = np.random.default_rng(7 + seed)
    s = min(p, 8) if s is None else s
    bstar = np.zeros(p)
    bstar[rng.choice(p, size=s, replace=False)] = rng.standard_normal(s) * 2
    return -(_A(p) @ bstar + 0.1 * rng.standard_normal(p))


def _same(f_stats, x, st, xo, tag=""):
    np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL, err_msg=str(tag))
    for key in ("passes", "full_passes", "visits", "converged"):
        assert f_stats[key] == st[key], (tag, key, f_stats, st)
    assert x.nzval2ind.tolist() == xo.nzval2ind.tolist(), tag


def _grad_bar(b):
    """The handle's gradient against A x + b: 1e-11 max(1, max|b|)."""
    return 1e-11 * max(1.0, float(np.abs(b).max()))


def _oracle_gradient(fo):
    """A x + b as the oracle's CDQuadraticLoss carries it (its r is A x)."""
    return fo.r + fo.y
