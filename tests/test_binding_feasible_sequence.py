"""feasibleLasso!(x, X::HipMatrix, ...) and refitLassoPath(path, X::HipMatrix, Y) of julia/CoordinateDescentHIP.jl, REPLAYED as
the exact sequences of C-ABI calls they make, the way tests/test_binding_call_sequence.py replays the rest of the binding
(whose replayed helper methods are used here as they stand: plain ctypes on libcdhip.so, nothing of api.py in between).
Results are compared with the restatement of lasso.jl:154-194 on the CPU oracle and with numpy's lstsq."""
import numpy as np
import pytest

import _feasible_oracle as FO
import test_binding_call_sequence as B
from test_binding_call_sequence import ccall, i64, ptr

pytestmark = pytest.mark.gpu

OPT_CD = dict(FO.CD, randomize=True)


def device_loadings(X):              # device_loadings!(out, X::HipMatrix)
    buf = np.zeros(X.p)
    ccall("cdh_loadings", X.handle, ptr(buf))
    return buf.astype(X.dtype)


def feasibleLasso_hip(x, X, y, lam0, init, sinit=5, sigmainit=1.0, maxIter=20, optTol=FO.OPT_TOL, optCD=OPT_CD):
    """feasibleLasso!(x, X::HipMatrix, y, λ0, options): the binding's own method."""
    f = B.Loss(B.CDH_LS, y, X)
    if init == "Screening":
        S = B.findLargestCorrelations(X, y, sinit)
        B.screening_ols(X, np.ascontiguousarray(np.nonzero(S)[0] + 1, dtype=np.int64))
        X.owner = f.r
    elif init == "InitStd":
        B.solve_resident(x, f, lam0 * sigmainit, B.stdX(X), optCD)
    elif init == "WarmStart":
        B.bind(f)
        B.push_iterate(f, x, True)
    else:
        raise B.ArgumentError("Incorrect initialization Symbol")
    gamma = device_loadings(X)
    rounds = 0
    for _ in range(maxIter):
        gamma_old = gamma.copy()
        B.solve_resident(x, f, lam0, gamma, optCD)
        gamma = device_loadings(X)         # (in place in the binding: g aliases it)
        rounds += 1
        if np.max(np.abs(gamma_old - gamma)) / np.max(gamma) < optTol:
            break
    B.pull_residual(f)
    return x, f.r, gamma, B.resid_std(X), rounds


def refitLassoPath_hip(betapath, X, Y):
    """refitLassoPath(path, X::HipMatrix, Y): the binding's own method."""
    out = {}
    ccall("cdh_set_loss", X.handle, B.i32(B.CDH_LS))
    yy = np.ascontiguousarray(Y, dtype=X.dtype)
    ccall("cdh_set_y", X.handle, ptr(yy))
    X.owner = None
    for beta in betapath:
        S = tuple(int(k) + 1 for k in np.nonzero(beta)[0])
        if S in out:
            continue
        ccall("cdh_initialize", X.handle, i64(X.p), i64(0), None, None)
        out[S] = B.screening_ols(X, np.array(S, dtype=np.int64)) if S else np.zeros(0)
    ccall("cdh_initialize", X.handle, i64(X.p), i64(0), None, None)
    X.synced = False
    return out


@pytest.mark.parametrize("init", FO.INITS)
def test_feasible_lasso_of_the_binding_matches_the_restatement(init):
    X, y, lam0 = FO.recipe(2)
    want = FO.solved(2, init)
    Xh = B.HipMatrix(X)
    x = B.SparseIterate(FO.P)
    copies = B.N_RESIDUAL_COPIES[0]
    x, r, gamma, sigma, rounds = feasibleLasso_hip(x, Xh, y, lam0, init)
    assert B.N_RESIDUAL_COPIES[0] == copies + 1            # f.r comes back once, for the LassoSolution
    assert rounds == len(want.stats)
    np.testing.assert_allclose(x.dense(), want.x.dense(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(sigma, want.sigma, rtol=1e-6)
    assert gamma.tobytes() == device_loadings(Xh).tobytes()   # the loadings after the last solve
    np.testing.assert_allclose(r, y - X @ x.dense(), rtol=0, atol=1e-9)
    Xh.close()


def test_refit_lasso_path_of_the_binding_is_lstsq_per_distinct_support():
    X, y, _ = FO.recipe(1)
    Xh = B.HipMatrix(X)
    sx = B.stdX(Xh)
    lmax = float(np.max(np.abs(X.T @ y) / FO.N / sx))
    lams, path = B.LassoPath_hip(Xh, y, [f * lmax for f in (1.05, 0.6, 0.3, 0.27, 0.1)],
                                 dict(maxIter=5000, optTol=1e-10, randomize=False))
    sups = [tuple(np.nonzero(b)[0] + 1) for b in path]
    assert sups[0] == () and sups[2] == sups[3] and len(set(sups)) == 3
    out = refitLassoPath_hip(path, Xh, y)
    assert sorted(out) == sorted(set(sups)) and out[()].shape == (0,)
    for S, coef in out.items():
        if S:
            np.testing.assert_allclose(coef, np.linalg.lstsq(X[:, np.array(S) - 1], y, rcond=None)[0], rtol=1e-9, atol=1e-12)
    Xh.close()
