"""The Cox lasso's front ends with strata and observation weights on the device -- coxLasso, coxLambdaMax, CoxLassoPath,
cvCoxLassoPath -- held to the numpy twin (tests/_cox_strata_numpy.py): the KKT conditions of the weighted stratified partial
likelihood at the solution, the twin's own IRLS loop (the same number of rounds), lambda_max at beta = 0, and the folds of a
cross-validated path against the twin's loop composed fold by fold.

Tolerances are those of tests/test_gpu_cox_cv.py: inner optTol 1e-12, IRLS optTol 1e-10 (OPT), the KKT tolerance
10 OPT max_j sum_k |X_j' diag(evA) X_k| / n, coefficients of two loops within 10 OPT, a log partial likelihood within
(n + 64) U of the sum of its terms' magnitudes.  One figure is new: with weights the folds' weights in cvm are the floats
sum v delta, which the device adds in its own order -- each within (n + 64) U of the host's sum -- so cvm, a weighted mean, is
held to the host's weighted mean within tol = 4 (n + 64) U max |fold_deviance| instead of to the last bit, and cvsd, the root
of a weighted variance that moves by at most 4 tol max |fold_deviance|, within the root of that (|sqrt a - sqrt b| <=
sqrt |a - b|).  Every case prints the figures it asserts on."""
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_numpy as CX
import _cox_strata_numpy as CS

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OPT = 1e-10
P = 8


def _opts():
    return cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)


def _irls():
    return cd.IRLSOptions(maxIter=100, optTol=OPT)


_DATA = {}


def _problem(n, seed):
    """(X, y = [time, status], time, status, offset, strata, weights as given, weights normalised to sum to n, lambda_max at
    beta = 0 by the twin): three strata with spread ids, weights uniform in [0.25, 4]; computed once and left unchanged."""
    if (n, seed) not in _DATA:
        X, t, s, off = CX.make_data(n, P, seed, decimals=1, censor=0.3, with_offset=True)
        rng = np.random.default_rng(seed + 100)
        g = rng.integers(0, 3, n) * 5 - 5
        v = rng.uniform(0.25, 4.0, n)
        vn = v * n / v.sum()
        q = CS.rows(np.zeros(n), off, t, s, 1e-300, 700.0, None, exact=True, strata=g, weights=vn)
        lmax = max(abs(math.fsum(X[:, j] * q["d"])) for j in range(P)) / n
        for a in (X, t, s, off, g, v, vn):
            a.setflags(write=False)
        _DATA[(n, seed)] = (X, np.c_[t, s], t, s, off, g, v, vn, lmax)
    return _DATA[(n, seed)]


def _kkt_ok(tag, X, beta, off, t, s, g, vn, lam, omega=None, train=None):
    v_off, v_on, H = CS.kkt(X, beta, off, t, s, lam, omega, train, g, vn)
    tol = 10 * OPT * H
    print(f"KKT {tag}: off the support {v_off:.2e} on it {v_on:.2e} (tolerance {tol:.2e}), nnz {np.count_nonzero(beta)}")
    assert v_off <= tol and v_on <= tol


def _ll(eta_lin, off, t, s, g, vn):
    """The weighted stratified log partial likelihood by the twin's exact sums, and the sum of its terms' magnitudes."""
    q = CS.rows(eta_lin, off, t, s, 1e-300, 700.0, None, exact=True, strata=g, weights=vn)
    return -math.fsum(q["nll"]), math.fsum(np.abs(q["nll"]))


def test_solution_meets_the_kkt_conditions_and_the_twin_loop_takes_the_same_rounds():
    """n = 300, p = 8, three strata, weights in [0.25, 4], an offset, times rounded to one decimal."""
    n = 300
    X, y, t, s, off, g, v, vn, lmax = _problem(n, 3)
    for frac in (0.5, 0.1):
        lam = frac * lmax
        sol = cd.coxLasso(X, y, lam, options=_opts(), irls=_irls(), offset=off, strata=g, weights=v)
        beta = sol.x.dense()
        assert sol.converged and sol.monotone and sol.capped == 0 and 1 <= sol.x.nnz < P
        assert isinstance(sol.events, float) and abs(sol.events - math.fsum(vn * s)) <= (n + 64) * U * math.fsum(vn * s)
        _kkt_ok(f"coxLasso strata+weights {frac} lambda_max", X, beta, off, t, s, g, vn, lam)
        l_t, scale = _ll(X @ beta, off, t, s, g, vn)
        assert abs(sol.nll - (-l_t / n)) <= (n + 65) * U * scale / n
        want, rounds, conv = CS.cox_lasso(X, t, s, off, lam, maxIter=100, optTol=OPT, strata=g, weights=vn)
        print(f"coxLasso strata+weights {frac} lambda_max: {sol.rounds} rounds, the twin's loop {rounds}; max|beta - beta_twin| "
              f"{np.max(np.abs(beta - want)):.2e}")
        assert conv and rounds == sol.rounds and np.max(np.abs(beta - want)) <= 10 * OPT
    # the unweighted, unstratified fit of the same data is another fit
    plain = cd.coxLasso(X, y, 0.1 * lmax, options=_opts(), irls=_irls(), offset=off)
    assert isinstance(plain.events, int) and np.max(np.abs(plain.x.dense() - beta)) > 1e-3


def test_lambda_max():
    n = 300
    X, y, t, s, off, g, v, vn, lmax = _problem(n, 3)
    f = cd.CDCoxLoss(y, X, off, strata=g, weights=v)
    np.testing.assert_array_equal(f.weights, vn)
    got = cd.coxLambdaMax(f)
    print(f"coxLambdaMax strata+weights: device {got:.17g} twin {lmax:.17g}, off by {abs(got - lmax) / lmax / U:.1f} U (bound {n + 64})")
    assert abs(got - lmax) <= (n + 64) * U * lmax
    f.close()
    above = cd.coxLasso(X, y, 1.0001 * lmax, options=_opts(), irls=_irls(), offset=off, strata=g, weights=v)
    below = cd.coxLasso(X, y, 0.999 * lmax, options=_opts(), irls=_irls(), offset=off, strata=g, weights=v)
    assert above.x.nnz == 0 and below.x.nnz >= 1 and above.converged and below.converged


def test_cv_path_against_the_twin_loop_composed_fold_by_fold():
    """n = 240, K = 3, 4 lambda, strata and weights.  A fold runs at lambda sqrt(n_k / n) on the scales _stdX!(w, X) of its 0/1
    weights -- NOT weighted by v -- warm-started along lambda (cvCoxLassoPath's docstring): the twin's loop does the same with
    the held-out rows at w = 0.  fold_deviance is the twin's -2 (l_all - l_train) / (held-out sum v delta) at the device's
    coefficients; the folds are weighted by those sums."""
    n, K = 240, 3
    X, y, t, s, off, g, v, vn, lmax = _problem(n, 7)
    lams = np.geomspace(0.7, 0.1, 4) * lmax
    ids = np.random.default_rng(0).permutation(n) % K
    kw = dict(options=_opts(), irls=_irls(), offset=off, strata=g, weights=v)
    res = cd.cvCoxLassoPath(X, y, lams, K=K, folds=ids, keep_fold_paths=True, **kw)
    assert isinstance(res, cd.CVCoxLassoPathResult) and res.fold_deviance.shape == (K, 4) and res.converged.all()
    events = np.bincount(ids, weights=s * vn, minlength=K)
    np.testing.assert_allclose(res.fold_events, events, rtol=4 * U, atol=0.0)
    np.testing.assert_array_equal(res.fold_sizes, np.bincount(ids))
    worst_b = worst_d = 0.0
    for k in range(K):
        tr = ids != k
        nk = int(tr.sum())
        sx = np.sqrt((X[tr] ** 2).sum(axis=0) / n)
        beta = np.zeros(P)
        for j in range(4):
            beta, rounds, conv = CS.cox_lasso(X, t, s, off, lams[j] * np.sqrt(nk / n), sx, beta, maxIter=100, optTol=OPT,
                                              train=tr, strata=g, weights=vn)
            b = res.fold_paths[k].betapath[j].dense()
            worst_b = max(worst_b, float(np.max(np.abs(b - beta))))
            assert conv and abs(rounds - res.rounds[k, j]) <= 1, (k, j, rounds, res.rounds[k, j])    # (a last step may straddle OPT)
            (l_all, _), (l_tr, scale_tr) = _ll(X @ b, off, t, s, g, vn), _ll((X @ b)[tr], off[tr], t[tr], s[tr], g[tr], vn[tr])
            want = -2.0 * (l_all - l_tr) / events[k]
            bound = (n + 64) * U * (abs(l_all) + abs(l_tr)) / events[k]
            worst_d = max(worst_d, abs(res.fold_deviance[k, j] - want) / bound)
            ev_tr = events.sum() - events[k]
            assert abs(res.train_deviance[k, j] - (-2.0 * l_tr / ev_tr)) <= (n + 64) * U * 2.0 * scale_tr / ev_tr
    print(f"cv strata+weights: max|beta_fold - beta_twin| {worst_b:.2e} (bound {10 * OPT:.0e}); fold_deviance off by {worst_d:.3f} "
          f"of its bound")
    assert worst_b <= 10 * OPT and worst_d <= 1.0
    wt = events / events.sum()
    tol = 4 * (n + 64) * U * np.max(np.abs(res.fold_deviance))
    cvm = wt @ res.fold_deviance
    assert np.max(np.abs(res.cvm - cvm)) <= tol
    assert np.max(np.abs(res.cvsd - np.sqrt(wt @ (res.fold_deviance - cvm) ** 2 / (K - 1)))) <= np.sqrt(4 * tol * np.max(np.abs(res.fold_deviance)))
    assert res.index_min == int(np.argmin(res.cvm)) and res.lambda_min == lams[res.index_min]
    # `path` is CoxLassoPath's result with the same arguments, bit for bit
    full = cd.CoxLassoPath(X, y, lams, **kw)
    assert res.path.rounds == full.rounds and res.path.nll == full.nll
    for a, b in zip(res.path.betapath, full.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())
    for lam, b in zip(lams, full.betapath):
        _kkt_ok(f"path lambda {lam:.4f}", X, b.dense(), off, t, s, g, vn, lam, np.sqrt((X * X).sum(axis=0) / n))


def test_cv_on_a_loss_keeps_its_strata_and_weights():
    n = 240
    X, y, t, s, off, g, v, vn, lmax = _problem(n, 7)
    f = cd.CDCoxLoss(y, X, off, strata=g, weights=v)
    res = cd.cvCoxLassoPath(f, None, [0.5 * lmax, 0.2 * lmax], K=3, options=_opts(), irls=_irls(), full_path=False)
    assert res.path is None and res.converged.all() and np.all(res.fold_deviance > 0) and res.fold_events.dtype == np.float64
    np.testing.assert_array_equal(f.strata, g)
    np.testing.assert_array_equal(f.weights, vn)
    sol = cd.coxLasso(f, None, 0.3 * lmax, options=_opts(), irls=_irls())
    assert sol.converged
    _kkt_ok("after cv, on the same handle", X, sol.x.dense(), off, t, s, g, vn, 0.3 * lmax)
    f.close()
