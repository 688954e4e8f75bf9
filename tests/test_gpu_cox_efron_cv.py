"""The Cox lasso's front ends with Efron ties on the device -- coxLambdaMax, coxLasso, CoxLassoPath and cvCoxLassoPath with
ties="efron" -- held to the numpy twin (tests/_cox_efron_numpy.py) on one small problem: n = 300, p = 8, times rounded to one
decimal, three strata, weights in [0.25, 4], an offset.  None of the front ends has arithmetic of its own for Efron: lambda_max,
the folds' held-out deviance 2 (l_all - l_train) and the lambda scaling of the folds follow from the step, and these tests
check that they do.

Tolerances are those of tests/test_gpu_cox_strata_cv.py and tests/test_gpu_cox_cv.py: inner optTol 1e-12, IRLS optTol 1e-10
(OPT), the KKT tolerance 10 OPT max_j sum_k |X_j' diag(evA) X_k| / n, coefficients of two loops within 10 OPT, a log partial
likelihood within (n + 64) U of the sum of its terms' magnitudes.  lambda_max is X'd / n at beta = 0 with the step's d: held to
the twin within the step test's bound on d, |dd_i| <= (4n + 66) U rho (dv_i + evA_i) (tests/test_gpu_cox_efron.py), carried
through the column sums, plus (n + 64) U of the sum's terms.  Every case prints the figures it asserts on."""
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_numpy as CX
import _cox_efron_numpy as CE

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OPT = 1e-10
P = 8
N = 300
SEED = 3


def _opts():
    return cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)


def _irls():
    return cd.IRLSOptions(maxIter=100, optTol=OPT)


_DATA = {}


def _problem():
    """(X, y, time, status, offset, strata, weights as given, weights normalised to sum to n); computed once, left unchanged."""
    if not _DATA:
        X, t, s, off = CX.make_data(N, P, SEED, decimals=1, censor=0.3, with_offset=True)
        rng = np.random.default_rng(SEED + 100)
        g = rng.integers(0, 3, N) * 5 - 5
        v = rng.uniform(0.25, 4.0, N)
        vn = v * N / v.sum()
        for a in (X, t, s, off, g, v, vn):
            a.setflags(write=False)
        _DATA["p"] = (X, np.c_[t, s], t, s, off, g, v, vn)
    return _DATA["p"]


def _kkt_ok(tag, X, beta, off, t, s, g, vn, lam, omega=None, train=None):
    v_off, v_on, H = CE.kkt(X, beta, off, t, s, lam, omega, train, g, vn)
    tol = 10 * OPT * H
    print(f"KKT {tag}: off the support {v_off:.2e} on it {v_on:.2e} (tolerance {tol:.2e}), nnz {np.count_nonzero(beta)}")
    assert v_off <= tol and v_on <= tol


def _lambda_max(X, off, t, s, g, vn, omega=None):
    """max_j |X_j'(dv - ev A)| / (n omega_j) at beta = 0 from the twin, and the bound of the module's docstring."""
    n = len(t)
    q = CE.rows(np.zeros(n), off, t, s, 1e-300, 700.0, strata=g, weights=vn, dtype=np.longdouble)
    om = np.ones(X.shape[1]) if omega is None else omega
    bd = (4 * n + 66) * U * q["rho"] * (q["delta"] + q["eA"])
    vals = [abs(math.fsum(X[:, j] * q["d"])) / (n * om[j]) for j in range(X.shape[1])]
    tols = [(math.fsum(np.abs(X[:, j]) * bd) + (n + 64) * U * math.fsum(np.abs(X[:, j] * q["d"]))) / (n * om[j]) for j in range(X.shape[1])]
    j = int(np.argmax(vals))
    return vals[j], max(tols)


def test_lambda_max_follows_from_the_step():
    X, y, t, s, off, g, v, vn = _problem()
    want, tol = _lambda_max(X, off, t, s, g, vn)
    f = cd.CDCoxLoss(y, X, off, strata=g, weights=v)
    breslow = cd.coxLambdaMax(f)
    f.set_ties("efron")
    got = cd.coxLambdaMax(f)
    f.close()
    print(f"coxLambdaMax efron: device {got:.17g} twin {want:.17g}, off by {abs(got - want):.2e} (bound {tol:.2e}); breslow {breslow:.17g}")
    assert abs(got - want) <= tol and abs(breslow - want) > 100 * tol
    kw = dict(options=_opts(), irls=_irls(), offset=off, strata=g, weights=v, ties="efron")
    above, below = cd.coxLasso(X, y, 1.0001 * want, **kw), cd.coxLasso(X, y, 0.999 * want, **kw)
    assert above.x.nnz == 0 and below.x.nnz >= 1 and above.converged and below.converged


def test_solution_meets_efrons_kkt_conditions_and_is_not_the_breslow_fit():
    X, y, t, s, off, g, v, vn = _problem()
    lmax, _ = _lambda_max(X, off, t, s, g, vn)
    kw = dict(options=_opts(), irls=_irls(), offset=off, strata=g, weights=v)
    for frac in (0.5, 0.1):
        lam = frac * lmax
        sol = cd.coxLasso(X, y, lam, ties="efron", **kw)
        beta = sol.x.dense()
        assert sol.converged and sol.monotone and sol.capped == 0 and 1 <= sol.x.nnz <= P
        _kkt_ok(f"coxLasso efron {frac} lambda_max", X, beta, off, t, s, g, vn, lam)
        # the nll the solution carries is the definition half's, within the step test's bound on the record's first slot
        want = CE.npl(X @ beta + off, t, s, g, vn) / N
        q = CE.rows(X @ beta, off, t, s, 1e-300, 700.0, strata=g, weights=vn, dtype=np.longdouble)
        mag = math.fsum(np.abs(q["mm"] * q["lg"]) + np.abs(q["delta"] * (X @ beta + off)))
        floor = math.fsum(q["mm"] * ((N + 11) * U * q["rho"] + 2 * U * np.abs(q["lg"])))
        assert abs(sol.nll - want) <= ((2 * N + 66) * U * mag + floor) / N
    # the keyword does something: Breslow's coefficients at the same lambda are another fit, by far more than the tolerance
    plain = cd.coxLasso(X, y, lam, **kw)
    named = cd.coxLasso(X, y, lam, ties="breslow", **kw)
    np.testing.assert_array_equal(plain.x.dense(), named.x.dense())
    gap = float(np.max(np.abs(plain.x.dense() - beta)))
    print(f"max|beta_efron - beta_breslow| {gap:.3e}: {gap / (10 * OPT):.0f} times the coefficient tolerance {10 * OPT:.0e}")
    assert gap >= 100 * 10 * OPT
    # on a loss: set_ties, and the keyword must agree with it
    f = cd.CDCoxLoss(y, X, off, strata=g, weights=v)
    f.set_ties("efron")
    with pytest.raises(cd.ArgumentError, match='ties="breslow" disagrees with the loss'):
        cd.coxLasso(f, None, lam, options=_opts(), irls=_irls())
    on_loss = cd.coxLasso(f, None, lam, options=_opts(), irls=_irls(), ties="efron")
    np.testing.assert_array_equal(on_loss.x.dense(), beta)
    assert f.ties == "efron"
    f.close()
    with pytest.raises(cd.ArgumentError, match="start-stop times"):        # Efron with start-stop times: refused at the handle too
        f3 = cd.CDCoxLoss(np.c_[t - 0.05, t, s], X, off)
        try:
            cd.check(f3._L.cdh_glm_set_cox_ties(f3._h, 1), f3._h)
        finally:
            f3.close()


def test_path_is_warm_started_and_monotone():
    X, y, t, s, off, g, v, vn = _problem()
    sx = np.sqrt((X * X).sum(axis=0) / N)
    lmax_s, _ = _lambda_max(X, off, t, s, g, vn, sx)
    lams = np.geomspace(0.9, 0.1, 5) * lmax_s
    kw = dict(options=_opts(), irls=_irls(), offset=off, strata=g, weights=v, ties="efron")
    res = cd.CoxLassoPath(X, y, lams, **kw)
    assert isinstance(res, cd.CoxLassoPathResult) and len(res.betapath) == 5 and all(res.converged)
    nnz = [b.nnz for b in res.betapath]
    assert nnz[0] >= 1 and nnz[-1] > nnz[0] and all(b >= a for a, b in zip(nnz, nnz[1:]))
    assert all(b < a for a, b in zip(res.nll, res.nll[1:]))                 # the fit improves as lambda falls
    for lam, b in zip(lams, res.betapath):
        _kkt_ok(f"efron path lambda {lam:.4f}", X, b.dense(), off, t, s, g, vn, lam, sx)
    cold = cd.coxLasso(X, y, lams[-1], sx, **kw)
    print(f"efron path rounds {res.rounds}; the last lambda from beta = 0: {cold.rounds}")
    assert res.rounds[-1] <= cold.rounds and np.max(np.abs(cold.x.dense() - res.betapath[-1].dense())) <= 10 * OPT
    assert cold.monotone


def test_cv_folds_follow_from_the_step():
    """K = 3, 4 lambda.  fold_deviance is the twin's 2 (npl_all - npl_train) / (held-out sum v delta) of Efron's likelihood -- its
    nll half, the plain loop over the event times -- at the device's fold coefficients; a fold's path is CoxLassoPath on its
    training rows alone at the scaled lambda: the fold runs at lambda sqrt(n_k / n) on the scales of its 0/1 weights, which for
    the loss (1 / n_k) sum of the training rows alone, its weights normalised to sum to n_k, is lambda (n_k / n) (V / V_k), V and
    V_k the sums of v over all rows and over the training rows (lambda itself without weights)."""
    X, y, t, s, off, g, v, vn = _problem()
    n, K = N, 3
    lmax, _ = _lambda_max(X, off, t, s, g, vn)
    lams = np.geomspace(0.7, 0.1, 4) * lmax
    ids = np.random.default_rng(0).permutation(n) % K
    kw = dict(options=_opts(), irls=_irls())
    res = cd.cvCoxLassoPath(X, y, lams, K=K, folds=ids, keep_fold_paths=True, offset=off, strata=g, weights=v, ties="efron", **kw)
    assert isinstance(res, cd.CVCoxLassoPathResult) and res.fold_deviance.shape == (K, 4) and res.converged.all()
    events = np.bincount(ids, weights=s * vn, minlength=K)
    np.testing.assert_allclose(res.fold_events, events, rtol=4 * U, atol=0.0)
    breslow = cd.cvCoxLassoPath(X, y, lams, K=K, folds=ids, offset=off, strata=g, weights=v, full_path=False, **kw)
    assert np.max(np.abs(breslow.fold_deviance - res.fold_deviance)) > 1e-6
    worst_b = worst_d = 0.0
    for k in range(K):
        tr = ids != k
        nk = int(tr.sum())
        scaled = lams * (nk / n) * (v.sum() / v[tr].sum())
        alone = cd.CoxLassoPath(np.asfortranarray(X[tr]), y[tr], scaled, offset=np.ascontiguousarray(off[tr]),
                                strata=np.ascontiguousarray(g[tr]), weights=np.ascontiguousarray(v[tr]), ties="efron", **kw)
        for j in range(4):
            b = res.fold_paths[k].betapath[j].dense()
            worst_b = max(worst_b, float(np.max(np.abs(b - alone.betapath[j].dense()))))
            eta = X @ b + off
            l_all, l_tr = -CE.npl(eta, t, s, g, vn), -CE.npl(eta, t, s, g, vn, tr)
            want = -2.0 * (l_all - l_tr) / events[k]
            bound = (n + 64) * U * (abs(l_all) + abs(l_tr)) / events[k]
            worst_d = max(worst_d, abs(res.fold_deviance[k, j] - want) / bound)
    print(f"cv efron: max|beta_fold - beta_alone| {worst_b:.2e} (bound {10 * OPT:.0e}); fold_deviance off by {worst_d:.3f} of its bound")
    assert worst_b <= 10 * OPT and worst_d <= 1.0
    full = cd.CoxLassoPath(X, y, lams, offset=off, strata=g, weights=v, ties="efron", **kw)
    for a, b in zip(res.path.betapath, full.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())
