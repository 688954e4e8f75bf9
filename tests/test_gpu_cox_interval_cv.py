"""The Cox lasso's front ends with start-stop times on the device -- coxLasso, coxLambdaMax, CoxLassoPath, cvCoxLassoPath with a
three-column y -- held to the numpy twin (tests/_cox_interval_numpy.py): the KKT conditions of the interval partial likelihood
at the solution, the twin's own IRLS loop (the same number of rounds), rows split at a cut against the unsplit rows, and the
folds of a cross-validated path, one fold id per SUBJECT, against the twin's loop composed fold by fold.

Tolerances are those of tests/test_gpu_cox_strata_cv.py: inner optTol 1e-12, IRLS optTol 1e-10 (OPT), the KKT tolerance
10 OPT max_j sum_k |X_j' diag(evA) X_k| / n, coefficients of two loops within 10 OPT, a log partial likelihood within
(n + 64) U of the sum of its terms' magnitudes, lambda_max within (n + 64) U of itself, cvm and cvsd as there.  The loss is
(1/rows) sum: a data set whose rows were split has more rows, so its lambda and lambda_max are the unsplit ones times
rows_unsplit / rows_split.  Every case prints the figures it asserts on."""
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_interval_numpy as CI

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OPT = 1e-10
P = 8


def _opts():
    return cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)


def _irls():
    return cd.IRLSOptions(maxIter=100, optTol=OPT)


def _subjects(n, seed, rounded=True):
    """n subjects whose stop time follows the hazard exp(X beta0 + offset) (so that the lasso has something to find), plus 0.05,
    rounded to one decimal; the start times by the tests' recipe (stop U(0, 0.9), 0 with probability 0.3, floored to a decimal)."""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, P)))
    off = rng.uniform(-0.5, 0.5, n)
    stop = rng.exponential(1.0, n) / np.exp(X @ CI.beta0(P) + off) + 0.05
    if rounded:
        stop = np.round(stop, 1)
    start = np.where(rng.random(n) < 0.3, 0.0, stop * rng.uniform(0.0, 0.9, n))
    if rounded:
        start = np.floor(start * 10.0) / 10.0
    status = (rng.random(n) < 0.7).astype(np.float64)
    assert np.all(start < stop) and status.any()
    return X, start, stop, status, off


def _lmax(X, off, start, stop, status, g=None, vn=None):
    n = len(stop)
    q = CI.rows(np.zeros(n), off, start, stop, status, 1e-300, 700.0, None, exact=True, strata=g, weights=vn)
    return max(abs(math.fsum(X[:, j] * q["d"])) for j in range(X.shape[1])) / n


def _kkt_ok(tag, X, beta, off, start, stop, status, g, vn, lam, omega=None, train=None):
    v_off, v_on, H = CI.kkt(X, beta, off, start, stop, status, lam, omega, train, g, vn)
    tol = 10 * OPT * H
    print(f"KKT {tag}: off the support {v_off:.2e} on it {v_on:.2e} (tolerance {tol:.2e}), nnz {np.count_nonzero(beta)}")
    assert v_off <= tol and v_on <= tol


def _ll(eta_lin, off, start, stop, status, g, vn):
    """The interval log partial likelihood by the twin's exact sums, and the sum of its terms' magnitudes."""
    q = CI.rows(eta_lin, off, start, stop, status, 1e-300, 700.0, None, exact=True, strata=g, weights=vn)
    return -math.fsum(q["nll"]), math.fsum(np.abs(q["nll"]))


def test_solution_meets_the_kkt_conditions_and_the_twin_loop_takes_the_same_rounds():
    """n = 300, p = 8, three strata, weights in [0.25, 4], an offset, start-stop times by the recipe (rounded: ties, and starts
    on event times)."""
    n = 300
    X, start, stop, status, off = _subjects(n, 3)
    rng = np.random.default_rng(103)
    g = rng.integers(0, 3, n) * 5 - 5
    v = rng.uniform(0.25, 4.0, n)
    vn = v * n / v.sum()
    y = np.c_[start, stop, status]
    assert np.isin(start, stop[status == 1.0]).any()
    lmax = _lmax(X, off, start, stop, status, g, vn)
    f = cd.CDCoxLoss(y, X, off, strata=g, weights=v)
    np.testing.assert_array_equal(f.start, start)
    got = cd.coxLambdaMax(f)
    f.close()
    print(f"coxLambdaMax interval: device {got:.17g} twin {lmax:.17g}, off by {abs(got - lmax) / lmax / U:.1f} U (bound {n + 64})")
    assert abs(got - lmax) <= (n + 64) * U * lmax
    for frac in (0.5, 0.1):
        lam = frac * lmax
        sol = cd.coxLasso(X, y, lam, options=_opts(), irls=_irls(), offset=off, strata=g, weights=v)
        beta = sol.x.dense()
        assert sol.converged and sol.monotone and sol.capped == 0 and 1 <= sol.x.nnz <= P
        _kkt_ok(f"coxLasso interval {frac} lambda_max", X, beta, off, start, stop, status, g, vn, lam)
        l_t, scale = _ll(X @ beta, off, start, stop, status, g, vn)
        assert abs(sol.nll - (-l_t / n)) <= (n + 65) * U * scale / n
        want, rounds, conv = CI.cox_lasso(X, start, stop, status, off, lam, maxIter=100, optTol=OPT, strata=g, weights=vn)
        print(f"coxLasso interval {frac} lambda_max: {sol.rounds} rounds, the twin's loop {rounds}; max|beta - beta_twin| "
              f"{np.max(np.abs(beta - want)):.2e}")
        assert conv and rounds == sol.rounds and np.max(np.abs(beta - want)) <= 10 * OPT
    # the fit that ignores the start times is another fit
    late = cd.coxLasso(X, y[:, 1:], 0.1 * lmax, options=_opts(), irls=_irls(), offset=off, strata=g, weights=v)
    assert np.max(np.abs(late.x.dense() - beta)) > 1e-3


def test_rows_split_at_a_cut_fit_the_unsplit_likelihood():
    """Every row (0, t] with t > c becomes (0, c] censored plus (c, t]: the same likelihood on more rows.  The split fit at
    lambda is the unsplit fit at lambda rows_split / rows: its beta meets the KKT conditions of the UNSPLIT likelihood there,
    and lambda_max of the two agree after the same scaling."""
    n = 200
    X, _, stop, status, off = _subjects(n, 23)
    for cut in (0.5, float(np.median(stop)) + 0.03):             # an event time of the rounded recipe, and a time between two
        X2, start2, stop2, status2, off2, _ = CI.split_rows(X, stop, status, off, cut)
        n2 = len(stop2)
        assert n2 > n + 20 and ((stop[status == 1.0] == cut).any() == (cut == 0.5))
        whole = cd.CDCoxLoss(np.c_[stop, status], X, off)
        parts = cd.CDCoxLoss(np.c_[start2, stop2, status2], X2, off2)
        a, b = cd.coxLambdaMax(whole), cd.coxLambdaMax(parts)
        whole.close()
        parts.close()
        print(f"lambda_max unsplit {a:.17g}, split x rows {b * n2 / n:.17g}: off by {abs(a - b * n2 / n) / a / U:.1f} U (bound {n2 + 64})")
        assert abs(a - b * n2 / n) <= (n2 + 64) * U * a
        lam = 0.2 * a
        sol = cd.coxLasso(X2, np.c_[start2, stop2, status2], lam * n / n2, options=_opts(), irls=_irls(), offset=off2)
        assert sol.converged and 1 <= sol.x.nnz < P
        _kkt_ok(f"split at {cut:.3f} against the unsplit likelihood", X, sol.x.dense(), off, None, stop, status, None, None, lam)
        ref = cd.coxLasso(X, np.c_[stop, status], lam, options=_opts(), irls=_irls(), offset=off)
        print(f"split at {cut:.3f}: max|beta_split - beta_unsplit| {np.max(np.abs(sol.x.dense() - ref.x.dense())):.2e}")


def _two_rows_a_subject(m, extra, seed):
    """m subjects by the recipe, `extra` of them cut in two at a decimal inside their interval (time-varying covariates: the
    second piece has a covariate of its own): -> X, start, stop, status, off, subject of every row."""
    X, start, stop, status, off = _subjects(m, seed)
    cut = np.round((start + stop) / 2.0, 1)
    can = np.nonzero((start < cut) & (cut < stop))[0][:extra]
    assert len(can) == extra
    rng = np.random.default_rng(seed + 1)
    X2 = X[can].copy()
    X2[:, 0] += rng.standard_normal(extra)                      # the covariate that changed at the cut
    stop1, status1 = stop.copy(), status.copy()
    stop1[can], status1[can] = cut[can], 0.0
    subject = np.r_[np.arange(m), can]
    return (np.asfortranarray(np.r_[X, X2]), np.r_[start, cut[can]], np.r_[stop1, stop[can]], np.r_[status1, status[can]],
            np.r_[off, off[can]], subject)


def test_cv_path_with_folds_by_subject_against_the_twin_loop():
    """n = 240 rows of 160 subjects, K = 3, 4 lambda, three strata and weights, both per subject; the folds are given per
    subject, so that a subject's rows share one.  A fold runs at lambda sqrt(n_k / n) on the scales _stdX!(w, X) of its 0/1
    weights, warm-started along lambda: the twin's loop does the same with the held-out rows at w = 0.  fold_deviance is the
    twin's -2 (l_all - l_train) / (held-out sum v delta) at the device's coefficients."""
    n, K = 240, 3
    X, start, stop, status, off, subject = _two_rows_a_subject(160, 80, 7)
    assert len(stop) == n
    rng = np.random.default_rng(107)
    g = (rng.integers(0, 3, 160) * 5 - 5)[subject]
    v = rng.uniform(0.25, 4.0, 160)[subject]
    vn = v * n / v.sum()
    ids = (rng.permutation(160) % K)[subject]
    y = np.c_[start, stop, status]
    lmax = _lmax(X, off, start, stop, status, g, vn)
    lams = np.geomspace(0.7, 0.1, 4) * lmax
    kw = dict(options=_opts(), irls=_irls(), offset=off, strata=g, weights=v)
    res = cd.cvCoxLassoPath(X, y, lams, K=K, folds=ids, keep_fold_paths=True, **kw)
    assert isinstance(res, cd.CVCoxLassoPathResult) and res.fold_deviance.shape == (K, 4) and res.converged.all()
    events = np.bincount(ids, weights=status * vn, minlength=K)
    np.testing.assert_allclose(res.fold_events, events, rtol=4 * U, atol=0.0)
    np.testing.assert_array_equal(res.fold_sizes, np.bincount(ids))
    worst_b = worst_d = 0.0
    for k in range(K):
        tr = ids != k
        nk = int(tr.sum())
        sx = np.sqrt((X[tr] ** 2).sum(axis=0) / n)
        beta = np.zeros(P)
        for j in range(4):
            beta, rounds, conv = CI.cox_lasso(X, start, stop, status, off, lams[j] * np.sqrt(nk / n), sx, beta, maxIter=100,
                                              optTol=OPT, train=tr, strata=g, weights=vn)
            b = res.fold_paths[k].betapath[j].dense()
            worst_b = max(worst_b, float(np.max(np.abs(b - beta))))
            assert conv and abs(rounds - res.rounds[k, j]) <= 1, (k, j, rounds, res.rounds[k, j])    # (a last step may straddle OPT)
            (l_all, _) = _ll(X @ b, off, start, stop, status, g, vn)
            (l_tr, scale_tr) = _ll((X @ b)[tr], off[tr], start[tr], stop[tr], status[tr], g[tr], vn[tr])
            want = -2.0 * (l_all - l_tr) / events[k]
            bound = (n + 64) * U * (abs(l_all) + abs(l_tr)) / events[k]
            worst_d = max(worst_d, abs(res.fold_deviance[k, j] - want) / bound)
            ev_tr = events.sum() - events[k]
            assert abs(res.train_deviance[k, j] - (-2.0 * l_tr / ev_tr)) <= (n + 64) * U * 2.0 * scale_tr / ev_tr
    print(f"cv interval: max|beta_fold - beta_twin| {worst_b:.2e} (bound {10 * OPT:.0e}); fold_deviance off by {worst_d:.3f} "
          f"of its bound")
    assert worst_b <= 10 * OPT and worst_d <= 1.0
    wt = events / events.sum()
    tol = 4 * (n + 64) * U * np.max(np.abs(res.fold_deviance))
    cvm = wt @ res.fold_deviance
    assert np.max(np.abs(res.cvm - cvm)) <= tol
    assert np.max(np.abs(res.cvsd - np.sqrt(wt @ (res.fold_deviance - cvm) ** 2 / (K - 1)))) <= np.sqrt(4 * tol * np.max(np.abs(res.fold_deviance)))
    # `path` is CoxLassoPath's result with the same arguments, bit for bit
    full = cd.CoxLassoPath(X, y, lams, **kw)
    assert res.path.rounds == full.rounds and res.path.nll == full.nll
    for a, b in zip(res.path.betapath, full.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())
    for lam, b in zip(lams, full.betapath):
        _kkt_ok(f"path lambda {lam:.4f}", X, b.dense(), off, start, stop, status, g, vn, lam, np.sqrt((X * X).sum(axis=0) / n))


def test_cv_on_a_loss_keeps_its_start_times():
    n = 240
    X, start, stop, status, off, subject = _two_rows_a_subject(160, 80, 7)
    ids = (np.random.default_rng(1).permutation(160) % 3)[subject]
    lmax = _lmax(X, off, start, stop, status)
    f = cd.CDCoxLoss(np.c_[start, stop, status], X, off)
    res = cd.cvCoxLassoPath(f, None, [0.5 * lmax, 0.2 * lmax], K=3, folds=ids, options=_opts(), irls=_irls(), full_path=False)
    assert res.path is None and res.converged.all() and np.all(res.fold_deviance > 0)
    np.testing.assert_array_equal(f.start, start)
    np.testing.assert_array_equal(f.time, stop)
    sol = cd.coxLasso(f, None, 0.3 * lmax, options=_opts(), irls=_irls())
    assert sol.converged
    _kkt_ok("after cv, on the same handle", X, sol.x.dense(), off, start, stop, status, None, None, 0.3 * lmax)
    f.close()
