"""A numpy twin of cvLogisticLassoPath, written from the definitions on tests/_logistic_numpy.py and the CPU oracle (not from
api.py, and NOT as the masked formulation the product runs): per fold the logistic path is fitted on the training rows ALONE
(X[~held], omega = their own column rms), then the deviance and the class error are evaluated on X[held].  The three cases
are the ones tests/test_gpu_glm.py solves; the twin's answers are computed once per case and shared.

Also here, for the row-by-row tests of the fold-aware step: what a held-out row counts as misclassified, and the masked route
itself on the oracle's weighted loss (tests/test_cv_logistic_host.py holds it to the training-rows-only fit)."""
import numpy as np

import oracle as O
import _cv_numpy as CV
import _logistic_numpy as LG

# name -> (n, p, planted coefficients, seed of make_data, intercept or None, K); fold ids default_rng(0).permutation(n) % K
CASES = {"257x20": (257, 20, 3, 1, None, 3), "300x12+b": (300, 12, 3, 7, 0.8, 4), "500x50": (500, 50, 5, 2, None, 5)}
FRACS12 = np.geomspace(0.9, 0.02, 12)
INDEX_MIN = {"257x20": 5, "300x12+b": 6, "500x50": 7}      # of the deviance curve; asserted in test_cv_logistic_host.py
_TWIN = {}


def miss(y, eta):
    """Per row y [eta <= 0] + (1 - y) [eta > 0]: glmnet's type.measure = "class" for labels in [0, 1]; eta = 0 predicts 0."""
    y, eta = np.asarray(y, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    return np.where(eta > 0.0, 1.0 - y, y)


def data(name):
    """-> (X, y, intercept?, K, fold ids, lambdas): 12 lambdas on geomspace(0.9, 0.02) of the standardised lambda_max."""
    n, p, s, seed, b0, K = CASES[name]
    icpt = b0 is not None
    X, y, _ = LG.make_data(n, p, s, seed, b0 or 0.0)
    sx = np.sqrt((X * X).sum(axis=0) / n)
    lams = FRACS12 * LG.lambda_max(X, y, sx, intercept=icpt)
    return X, y, icpt, K, CV.fold_ids(n, K, 0), lams


def cv(name, optTol=1e-10):
    """The twin's cross-validation of a case -> dict(paths[k] = [(beta, b0, rounds)], fold_deviance, train_deviance, fold_class,
    min_abs_eta[k, j] over the held-out rows, sizes, and per measure (cvm, cvsd, index_min, index_1se))."""
    if name in _TWIN:
        return _TWIN[name]
    X, y, icpt, K, ids, lams = data(name)
    m = len(lams)
    dev, tdev, cls, amin = np.zeros((K, m)), np.zeros((K, m)), np.zeros((K, m)), np.zeros((K, m))
    paths = []
    for k in range(K):
        held = ids == k
        Xt, yt = np.asfortranarray(X[~held]), y[~held]           # the training rows only
        Xh, yh = X[held], y[held]
        path = LG.logistic_path(Xt, yt, lams, True, optTol=optTol, intercept=icpt)
        paths.append(path)
        for j, (b, b0, _) in enumerate(path):
            eh, et = Xh @ b + b0, Xt @ b + b0
            dev[k, j] = 2.0 * np.mean(LG.rows(yh, eh, 0.25)[3])
            tdev[k, j] = 2.0 * np.mean(LG.rows(yt, et, 0.25)[3])
            cls[k, j] = np.mean(miss(yh, eh))
            amin[k, j] = np.min(np.abs(eh))
    sizes = np.bincount(ids, minlength=K)
    out = dict(paths=paths, fold_deviance=dev, train_deviance=tdev, fold_class=cls, min_abs_eta=amin, sizes=sizes)
    for measure, err in (("deviance", dev), ("class", cls)):
        cvm, cvsd = CV.cv_curve(sizes, err)
        out[measure] = (cvm, cvsd) + CV.select(lams, cvm, cvsd)
    _TWIN[name] = out
    return out


def masked_lasso(X, y, held, lam, optTol=1e-7, wmin=1e-5, maxIter=25, intercept=False, rounds_exact=None):
    """The route the product takes, on the oracle's CDWeightedLSLoss over ALL n rows: rows of LG.rows, then w = 0 and z = eta
    on the held-out rows, omega = sqrt(sum_train x^2 / n) (the intercept's 0), lambda sqrt(n_k / n); started at zero (the
    intercept at the logit of the training rows' mean label).  -> (beta (length p), b0, rounds)."""
    n, p = X.shape
    X1 = LG.with_ones(X) if intercept else X
    nk = int((~held).sum())
    om = np.sqrt((X[~held] ** 2).sum(axis=0) / n)
    om1 = np.r_[om, 0.0] if intercept else om
    beta = np.zeros(X1.shape[1])
    if intercept:
        ybar = np.mean(y[~held])
        beta[p] = np.log(ybar / (1.0 - ybar))
    x = O.SparseIterate(X1.shape[1], beta)
    g = O.ProxL1(lam * np.sqrt(nk / n), om1)
    options = O.CDOptions(maxIter=100000, optTol=1e-12, randomize=False)
    rounds = 0
    for _ in range(maxIter if rounds_exact is None else rounds_exact):
        eta = X1 @ beta
        w, z, _, _, _ = LG.rows(y, eta, wmin)
        w, z = np.where(held, 0.0, w), np.where(held, eta, z)
        O.coordinateDescent_(x, O.CDWeightedLSLoss(z, X1, w), g, options)
        new = x.dense()
        rounds += 1
        step = float(np.max(np.abs(new - beta)))
        beta = new
        if rounds_exact is None and step < optTol:
            break
    return beta[:p].copy(), float(beta[p]) if intercept else 0.0, rounds
