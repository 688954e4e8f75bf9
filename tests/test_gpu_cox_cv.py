"""The Cox lasso's front ends on the device -- coxLasso, coxLambdaMax, CoxLassoPath, cvCoxLassoPath -- held to the numpy twin's
own gradient (tests/_cox_numpy.py): the KKT conditions of F at every solution, the same IRLS rounds composed on the host
through cdh_get_residual, cdh_set_y and cdh_set_obs_weights, lambda_max at beta = 0, the folds of a cross-validated path against
paths on the training rows alone, and the grouped partial-likelihood deviance of the held-out rows.

Inner optTol 1e-12, IRLS optTol 1e-10 (OPT below).  The KKT tolerance is 10 OPT max_j sum_k |X_j' diag(eA) X_k| / n: eA
dominates the true Hessian of the partial likelihood, so this bounds what a move of beta by OPT can do to the gradient; the factor
10 is the slack the Poisson solve tests give two nested tolerances.  Every case prints the figures it asserts on."""
import ctypes as C
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_numpy as CX

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BAD = cd._lib.CDH_BAD_ARG
OPT = 1e-10


def _opts():
    return cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)


def _irls():
    return cd.IRLSOptions(maxIter=100, optTol=OPT)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_DATA = {}


def _problem(n, seed):
    """(X, y = [time, status], time, status, offset, lambda_max at beta = 0 by the twin), computed once and left unchanged."""
    if (n, seed) not in _DATA:
        X, t, s, off = CX.make_data(n, 8, seed, decimals=1, censor=0.3, with_offset=True)
        q = CX.rows(np.zeros(n), off, t, s, 1e-300, 700.0, None, exact=True)
        lmax = max(abs(math.fsum(X[:, j] * q["d"])) for j in range(8)) / n
        for a in (X, t, s, off):
            a.setflags(write=False)
        _DATA[(n, seed)] = (X, np.c_[t, s], t, s, off, lmax)
    return _DATA[(n, seed)]


def _kkt_ok(tag, X, beta, off, t, s, lam, omega=None, train=None):
    v_off, v_on, H = CX.kkt(X, beta, off, t, s, lam, omega, train)
    tol = 10 * OPT * H
    print(f"KKT {tag}: off the support {v_off:.2e} on it {v_on:.2e} (tolerance {tol:.2e}), nnz {np.count_nonzero(beta)}")
    assert v_off <= tol and v_on <= tol


def _ll(eta_lin, off, t, s):
    """The log partial likelihood by the twin's exact sums, and the scale of its rounding: the sum of its terms
    delta (log S - eta), which are all >= 0 -- here, with hundreds of events, never a sum of roundings alone."""
    q = CX.rows(eta_lin, off, t, s, 1e-300, 700.0, None, exact=True)
    return -math.fsum(q["nll"]), math.fsum(np.abs(q["nll"]))


def _composed(f, t, s, off, lam, irls):
    """coxLasso_'s rounds with the twin's step on the host: three n-sized transfers and an initialize! per round."""
    L, h, n = f._L, f._h, f.n
    x, r, z = cd.SparseIterate(f.p), np.zeros(n), np.zeros(n)
    cd.check(L.cdh_set_y(h, _vp(z)), h)
    f._synced = None
    cd.initialize_(f, x)
    beta, rounds = x.dense(), 0
    for rounds in range(1, irls.maxIter + 1):
        cd.check(L.cdh_get_residual(h, _vp(r)), h)
        q = CX.rows(z - r, off, t, s, irls.wmin, irls.etaMax)
        z, w = np.ascontiguousarray(q["z"]), np.ascontiguousarray(q["w"])
        cd.check(L.cdh_set_y(h, _vp(z)), h)
        cd.check(L.cdh_set_obs_weights(h, _vp(w)), h)
        f._synced = None
        cd.initialize_(f, x)
        cd.coordinateDescent_(x, f, cd.ProxL1(lam), _opts())
        beta, old = x.dense(), beta
        if np.max(np.abs(beta - old)) < irls.optTol:
            break
    return beta, rounds


# ---- solves ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", (0.5, 0.1))
def test_solution_meets_the_kkt_conditions_and_the_composed_loop(frac):
    """n = 400, p = 8, times rounded to one decimal, three rows in ten censored, an offset."""
    X, y, t, s, off, lmax = _problem(400, 3)
    lam = frac * lmax
    sol = cd.coxLasso(X, y, lam, options=_opts(), irls=_irls(), offset=off)
    beta = sol.x.dense()
    assert sol.converged and sol.monotone and sol.capped == 0 and sol.events == int(s.sum()) and 1 <= sol.x.nnz < 8
    _kkt_ok(f"coxLasso {frac} lambda_max", X, beta, off, t, s, lam)
    l_t, scale = _ll(X @ beta, off, t, s)
    assert abs(sol.nll - (-l_t / 400)) <= (400 + 64) * U * scale / 400
    f = cd.CDCoxLoss(y, X, off)
    l_0, scale_0 = _ll(np.zeros(400), off, t, s)
    assert abs(f.objective(cd.ProxL1(lam)) - (-l_0 / 400)) <= (400 + 64) * U * scale_0 / 400     # (read-only: a fresh handle holds beta = 0)
    got, rounds = _composed(f, t, s, off, lam, _irls())
    f.close()
    print(f"coxLasso {frac} lambda_max: {sol.rounds} rounds, composed on the host {rounds}; max|beta - beta_composed| "
          f"{np.max(np.abs(beta - got)):.2e}")
    assert rounds == sol.rounds and np.max(np.abs(beta - got)) <= 10 * OPT


def test_lambda_max():
    X, y, t, s, off, lmax = _problem(400, 3)
    n = 400
    f = cd.CDCoxLoss(y, X, off)
    got = cd.coxLambdaMax(f)
    print(f"coxLambdaMax: device {got:.17g} twin {lmax:.17g}, off by {abs(got - lmax) / lmax / U:.1f} U (bound {n + 64})")
    assert abs(got - lmax) <= (n + 64) * U * lmax
    om = np.linspace(0.5, 2.0, 8)
    q = CX.rows(np.zeros(n), off, t, s, 1e-300, 700.0, None, exact=True)
    want = max(abs(math.fsum(X[:, j] * q["d"])) / (n * om[j]) for j in range(8))
    assert abs(cd.coxLambdaMax(f, om) - want) <= (n + 64) * U * want
    f.close()
    above = cd.coxLasso(X, y, 1.0001 * lmax, options=_opts(), irls=_irls(), offset=off)
    below = cd.coxLasso(X, y, 0.999 * lmax, options=_opts(), irls=_irls(), offset=off)
    assert above.x.nnz == 0 and below.x.nnz >= 1 and above.converged and below.converged


def test_path_is_warm_started_and_every_solution_meets_kkt():
    X, y, t, s, off, lmax = _problem(400, 3)
    n = 400
    sx = np.sqrt((X * X).sum(axis=0) / n)
    f = cd.CDCoxLoss(y, X, off)
    lmax_s = cd.coxLambdaMax(f, sx)
    f.close()
    lams = np.geomspace(0.9, 0.05, 8) * lmax_s
    res = cd.CoxLassoPath(X, y, lams, _opts(), _irls(), offset=off)
    assert isinstance(res, cd.CoxLassoPathResult) and len(res.betapath) == 8 and all(res.converged)
    assert res.intercepts == [None] * 8 and len(res.nll) == 8
    nnz = [b.nnz for b in res.betapath]
    assert nnz[0] >= 1 and nnz[-1] > nnz[0] and all(b >= a for a, b in zip(nnz, nnz[1:]))
    assert all(b < a for a, b in zip(res.nll, res.nll[1:]))                 # the fit improves as lambda falls
    for lam, b in zip(lams, res.betapath):
        _kkt_ok(f"path lambda {lam:.4f}", X, b.dense(), off, t, s, lam, sx)
    # warm-started: the last solve of the path takes no more rounds than the same solve from beta = 0, and ends where it ends
    cold = cd.coxLasso(X, y, lams[-1], sx, _opts(), _irls(), offset=off)
    print(f"path rounds {res.rounds}; the last lambda from beta = 0: {cold.rounds}")
    assert res.rounds[-1] <= cold.rounds and np.max(np.abs(cold.x.dense() - res.betapath[-1].dense())) <= 10 * OPT
    cut = cd.CoxLassoPath(X, y, lams, _opts(), _irls(), max_hat_s=nnz[2], offset=off)
    stop = next(i for i, v in enumerate(nnz) if v > nnz[2])
    assert len(cut.betapath) == stop + 1 == len(cut.lambdapath) and cut.betapath[-1].nnz == nnz[stop]


# ---- cross-validation ------------------------------------------------------------------------------------------------------------
def test_cv_path_against_paths_on_the_training_rows_alone():
    """n = 600, K = 3, 5 lambda.  Per fold the coefficients are CoxLassoPath's on a fresh loss of the training rows alone at the
    same lambda (the fold runs at lambda sqrt(n_k / n) on weighted scales: cvCoxLassoPath's docstring); fold_deviance is the
    twin's -2 (l_all - l_train) / events_k at those coefficients."""
    X, y, t, s, off, lmax = _problem(600, 7)
    n, K = 600, 3
    lams = np.geomspace(0.7, 0.05, 5) * lmax
    ids = np.random.default_rng(0).permutation(n) % K
    res = cd.cvCoxLassoPath(X, y, lams, K=K, folds=ids, options=_opts(), irls=_irls(), offset=off, keep_fold_paths=True)
    assert isinstance(res, cd.CVCoxLassoPathResult) and res.fold_deviance.shape == (K, 5) and res.converged.all()
    events = np.array([int(s[ids == k].sum()) for k in range(K)])
    np.testing.assert_array_equal(res.fold_events, events)
    np.testing.assert_array_equal(res.fold_sizes, np.bincount(ids))
    worst_b = worst_d = 0.0
    for k in range(K):
        tr = ids != k
        alone = cd.CoxLassoPath(np.asfortranarray(X[tr]), y[tr], lams, _opts(), _irls(), offset=np.ascontiguousarray(off[tr]))
        for j in range(5):
            b = res.fold_paths[k].betapath[j].dense()
            worst_b = max(worst_b, float(np.max(np.abs(b - alone.betapath[j].dense()))))
            (l_all, _), (l_tr, scale_tr) = _ll(X @ b, off, t, s), _ll((X @ b)[tr], off[tr], t[tr], s[tr])
            want = -2.0 * (l_all - l_tr) / events[k]
            bound = (n + 64) * U * (abs(l_all) + abs(l_tr)) / events[k]
            worst_d = max(worst_d, abs(res.fold_deviance[k, j] - want) / bound)
            ev_tr = s.sum() - events[k]
            assert abs(res.train_deviance[k, j] - (-2.0 * l_tr / ev_tr)) <= (n + 64) * U * 2.0 * scale_tr / ev_tr
        assert res.fold_paths[k].rounds == list(res.rounds[k])
    print(f"cv: max|beta_fold - beta_alone| {worst_b:.2e} (bound {10 * OPT:.0e}); fold_deviance off by {worst_d:.3f} of its bound")
    assert worst_b <= 10 * OPT and worst_d <= 1.0
    wt = events / events.sum()
    np.testing.assert_allclose(res.cvm, wt @ res.fold_deviance, rtol=1e-15)
    np.testing.assert_allclose(res.cvsd, np.sqrt(wt @ (res.fold_deviance - res.cvm) ** 2 / (K - 1)), rtol=1e-14)
    assert res.index_min == int(np.argmin(res.cvm)) and res.lambda_min == lams[res.index_min]
    # `path` is CoxLassoPath's result, bit for bit
    full = cd.CoxLassoPath(X, y, lams, _opts(), _irls(), offset=off)
    assert res.path.rounds == full.rounds and res.path.nll == full.nll
    for a, b in zip(res.path.betapath, full.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())


def test_cv_on_a_loss_drops_the_folds_and_refuses_eventless_folds():
    X, y, t, s, off, lmax = _problem(600, 7)
    n = 600
    f = cd.CDCoxLoss(y, X, off)
    res = cd.cvCoxLassoPath(f, None, [0.5 * lmax, 0.2 * lmax], K=3, options=_opts(), irls=_irls(), full_path=False)
    assert res.path is None and res.fold_paths is None and res.converged.all() and np.all(res.fold_deviance > 0)
    out = np.zeros(5)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    assert f._L.cdh_glm_cox_irls(f._h, 0, 0, 1e-5, 50.0, po) == BAD          # the folds are gone
    assert b"cdh_set_folds" in f._L.cdh_last_error(f._h)
    assert f._L.cdh_glm_cox_irls(f._h, -1, 0, 1e-5, 50.0, po) == cd._lib.CDH_OK
    ids = np.arange(n) % 3
    lone = np.zeros(n)
    lone[[0, 3]] = 1.0                                           # every event in fold 0: folds 1 and 2 hold none
    g = cd.CDCoxLoss(np.c_[t, lone], X)
    with pytest.raises(cd.ArgumentError, match="holds every event|holds no event"):
        cd.cvCoxLassoPath(g, None, [0.1], K=3, folds=ids)
    assert g._L.cdh_glm_cox_irls(g._h, 0, 0, 1e-5, 50.0, po) == BAD          # refused before any fold was set
    g.close()
    # the handle serves the ordinary front end afterwards
    sol = cd.coxLasso(f, None, 0.3 * lmax, options=_opts(), irls=_irls())
    assert sol.converged
    _kkt_ok("after cv, on the same handle", X, sol.x.dense(), off, t, s, 0.3 * lmax)
    f.close()
