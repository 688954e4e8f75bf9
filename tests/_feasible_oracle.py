"""feasibleLasso! (src/lasso.jl:154-194) restated on the CPU oracle, as the reference intends it (its `Array{T}(p)` at
:164-165 and its `LassoSolution(...)` call at :193 do not run on Julia >= 1.0): the yardstick of tests/test_gpu_feasible.py
and of tests/test_feasible_oracle.py, which checks the restatement itself.  Also the data recipe both share."""
from dataclasses import dataclass

import numpy as np

import oracle as O

N, P = 300, 40
SEEDS = (1, 2, 3)
INITS = ("Screening", "InitStd", "WarmStart")
OPT_TOL = 1e-2                                   # IterLassoOptions' default
CD = dict(maxIter=5000, optTol=1e-8, seed=4)


def recipe(seed, n=N, p=P):
    """Heteroscedastic noise on a 5-sparse signal: y = X beta* + (0.5 + |X_i1|) eps."""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    beta = np.zeros(p)
    beta[:5] = (2.0, -1.5, 1.0, -1.0, 0.8)
    y = X @ beta + (0.5 + np.abs(X[:, 0])) * rng.standard_normal(n)
    lam0 = 1.1 * np.sqrt(2.0 * np.log(2.0 * p / 0.05) / n)
    return X, y, float(lam0)


def get_loadings(X, e):
    """_getLoadings!(out, X, e) (src/utils.jl:153-164)."""
    X, e = np.asarray(X, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return np.sqrt(np.sum((X * e[:, None]) ** 2, axis=0) / X.shape[0])


@dataclass
class Feasible:
    x: O.SparseIterate
    loadings: np.ndarray          # computed after the last solve: what the returned penalty aliases (:181, :186)
    used: np.ndarray              # the loadings the last solve ran with
    stats: list                   # max|Γold - Γ| / max Γ of every round
    residuals: np.ndarray
    sigma: float


def feasible_lasso(x, X, y, lam0, init="Screening", maxIter=20, optTol=OPT_TOL, sinit=5, sigmainit=1.0, cd=None):
    ocd = O.CDOptions(**(cd or CD))
    y = np.asarray(y, dtype=np.float64)
    f = O.CDLeastSquaresLoss(y, X)
    if init == "Screening":
        f.r[:] = O.findInitResiduals(X, y, sinit)                                   # :169
    elif init == "InitStd":
        O.coordinateDescent_(x, f, O.ProxL1(lam0 * sigmainit, O.stdX(X)), ocd)      # :171-173
    elif init == "WarmStart":
        O.initialize_(f, x)                                                         # :175
    else:
        raise ValueError("ArgumentError: Incorrect initialization Symbol")
    gamma = get_loadings(X, f.r)                                                    # :179
    stats, used = [], gamma
    for _ in range(maxIter):
        used = gamma
        O.coordinateDescent_(x, f, O.ProxL1(lam0, gamma), ocd)                      # :185
        gamma = get_loadings(X, f.r)                                                # :186
        stats.append(float(np.max(np.abs(used - gamma)) / np.max(gamma)))           # :188
        if stats[-1] < optTol:
            break
    return Feasible(x, gamma, used, stats, f.r.copy(), float(np.std(f.r, ddof=1)))


_CACHE = {}


def solved(seed, init, **kw):
    """The restatement's run of the recipe, computed once per (seed, init, options) and shared: callers leave it unchanged."""
    key = (seed, init, tuple(sorted(kw.items())))
    if key not in _CACHE:
        X, y, lam0 = recipe(seed)
        _CACHE[key] = feasible_lasso(O.SparseIterate(P), X, y, lam0, init=init, **kw)
    return _CACHE[key]
