"""A numpy twin of the logistic and the Poisson lasso with observation weights, built on tests/_logistic_numpy.py and
tests/_poisson_numpy.py by import (their row functions are the unweighted step) and on the CPU oracle's CDWeightedLSLoss /
coordinateDescent_; written from the definitions, not from api.py.  The weights v_i > 0 are normalised to sum to n and the
objective is
    F(beta) = (1/n) sum_i v_i nll_i + lambda0 sum_j omega_j |beta_j|,
nll_i the family's own.  A row's step is the unweighted one -- r and z unchanged -- and its working weight v_i w_i, w_i the
family's weight already clamped at wmin, one rounded multiplication.  The records keep the layouts of the unweighted steps: the
nll, sum w, the held-out nll and both deviances weighted by v, the held-out misclassification sum v miss, the clamped and capped
rows counted.  The penalty scales stay the unweighted root mean squares over the rows present.

A family is "binomial" or "poisson"; o is the offset of the Poisson family (None: zeros; ignored by the binomial one).

The cross-validation twin goes by ROW SUBSETTING: fold k's path is fitted on X[train] alone, with the training rows' weights
renormalised to sum to n_k, and evaluated on X[held] -- not by the fold byte and the lambda scale the product runs.
fold_scale() is that scale; masked_lasso() the product's route on the oracle's loss, which the host tests hold to the subset
fit."""
import numpy as np

import oracle as O
import _cv_numpy as CV
import _cv_logistic_numpy as CVL
import _logistic_numpy as LG
import _poisson_numpy as PN

U = 2.0 ** -53
WMIN, ETA_MAX = PN.WMIN, PN.ETA_MAX


def normalise(v):
    """v n / sum v: what the front ends store."""
    v = np.asarray(v, dtype=np.float64)
    return v * len(v) / v.sum()


def rows(family, y, eta_lin, o, v, wmin=WMIN, eta_max=ETA_MAX):
    """-> dict(w, z, r, nll, dev, clamped, capped, w_fam, eta): the unweighted twin's row with w = v * w_fam.  eta is the full
    predictor (with the offset); dev is 2 nll for the binomial family; capped all False there."""
    eta_lin = np.asarray(eta_lin, dtype=np.float64)
    if family == "binomial":
        w, z, r, nll, clamped = LG.rows(y, eta_lin, wmin)
        dev, capped, eta = 2.0 * nll, np.zeros(len(eta_lin), dtype=bool), eta_lin
    else:
        w, z, r, nll, dev, clamped, capped = PN.rows(y, eta_lin, o, wmin, eta_max)
        eta = eta_lin + (0.0 if o is None else o)
    return dict(w=np.asarray(v) * w, z=z, r=r, nll=nll, dev=dev, clamped=clamped, capped=capped, w_fam=w, eta=eta)


def record(family, y, eta_lin, o, v, held=None, wmin=WMIN, eta_max=ETA_MAX):
    """The step's record and, per entry, the rows' terms it sums (zeros where a row does not enter): -> (record, terms).
    binomial: (sum_train v nll, sum_train w, clamped training rows, sum_held v nll, sum_held v miss);
    poisson: (sum_train v nll, sum_train w, clamped training rows, capped live rows, sum_held v dev, sum_train v dev)."""
    n = len(y)
    held = np.zeros(n, dtype=bool) if held is None else held
    train = ~held
    o_ = rows(family, y, eta_lin, o, v, wmin, eta_max)
    vn = v * o_["nll"]
    if family == "binomial":
        vm = v * CVL.miss(y, eta_lin)
        terms = [np.where(train, vn, 0.0), np.where(train, o_["w"], 0.0), (train & o_["clamped"]).astype(float),
                 np.where(held, vn, 0.0), np.where(held, vm, 0.0)]
    else:
        vd = v * o_["dev"]
        terms = [np.where(train, vn, 0.0), np.where(train, o_["w"], 0.0), (train & o_["clamped"]).astype(float),
                 o_["capped"].astype(float), np.where(held, vd, 0.0), np.where(train, vd, 0.0)]
    return np.array([t.sum() for t in terms]), terms


def _lin(X, beta, b0):
    return X @ beta + b0


def smooth(family, X, y, o, v, beta, b0=0.0):
    """(1/n) sum v nll at beta: the smooth part of F (wmin does not enter nll; eta is not capped here)."""
    return float(np.sum(v * rows(family, y, _lin(X, beta, b0), o, v, 1e-300, 700.0)["nll"]) / len(y))


def objective(family, X, y, o, v, beta, lam, omega=None, b0=0.0):
    om = np.ones(len(beta)) if omega is None else omega
    return smooth(family, X, y, o, v, beta, b0) + float(lam * np.sum(om * np.abs(beta)))


def mean(family, eta):
    return LG.prob(eta) if family == "binomial" else np.exp(eta)


def gradient(family, X, y, o, v, beta, b0=0.0):
    """d smooth / d beta = -X'(v (y - mu)) / n."""
    eta = _lin(X, beta, b0) + (0.0 if (o is None or family == "binomial") else o)
    return -(X.T @ (v * (y - mean(family, eta)))) / len(y)


def diagonal(family, X, y, o, v, beta, b0=0.0):
    """The diagonal of the Hessian of smooth: sum_i v_i w_i x_ij^2 / n with the unclamped family weights -- what the stored
    working weights v w stand for."""
    w = rows(family, y, _lin(X, beta, b0), o, v, 1e-300, 700.0)["w"]
    return (X * X).T @ w / len(y)


def null_intercept(family, y, o, v):
    """logit(sum vy / sum v), or log(sum vy / sum v e^o)."""
    if family == "binomial":
        ybar = np.sum(v * y) / np.sum(v)
        return float(np.log(ybar / (1.0 - ybar)))
    return float(np.log(np.sum(v * y) / (np.sum(v) if o is None else np.sum(v * np.exp(o)))))


def lambda_max(family, X, y, o, v, omega=None, intercept=False):
    """max_j |X_j'(v (y - mu))| / (n omega_j) at the null model."""
    b0 = null_intercept(family, y, o, v) if intercept else 0.0
    t = np.abs(gradient(family, X, y, o, v, np.zeros(X.shape[1]), b0))
    return float(np.max(t if omega is None else t / omega))


def glm_lasso(family, X, y, o, v, lam, omega=None, options=None, maxIter=25, optTol=1e-7, wmin=WMIN, eta_max=ETA_MAX,
              beta0=None, intercept=False):
    """The IRLS loop of the unweighted twins with v w for w and the weighted objective.  -> (beta (length p), b0, rounds,
    converged, largest rise of F between two rounds).  beta0: warm start, length p (+ 1)."""
    n, p = X.shape
    X1 = LG.with_ones(X) if intercept else X
    p1 = X1.shape[1]
    om = np.ones(p) if omega is None else np.asarray(omega, dtype=np.float64)
    om1 = np.r_[om, 0.0] if intercept else om
    options = options or O.CDOptions(maxIter=100000, optTol=1e-12, randomize=False)
    if beta0 is None:
        beta = np.zeros(p1)
        if intercept:
            beta[p] = null_intercept(family, y, o, v)
    else:
        beta = np.array(beta0, dtype=np.float64)
    x = O.SparseIterate(p1, beta)
    g = O.ProxL1(lam, om1)
    F = lambda b: float(np.sum(v * rows(family, y, X1 @ b, o, v, wmin, eta_max)["nll"]) / n + lam * np.sum(om1 * np.abs(b)))  # noqa: E731
    rise, Fprev, converged, rounds = -np.inf, F(beta), False, 0
    for _ in range(maxIter):
        o_ = rows(family, y, X1 @ beta, o, v, wmin, eta_max)
        O.coordinateDescent_(x, O.CDWeightedLSLoss(o_["z"], X1, o_["w"]), g, options)
        new = x.dense()
        rounds += 1
        Fnew = F(new)
        rise, Fprev = max(rise, Fnew - Fprev), Fnew
        step = float(np.max(np.abs(new - beta)))
        beta = new
        if step < optTol:
            converged = True
            break
    return (beta[:p].copy(), float(beta[p]) if intercept else 0.0, rounds, converged, rise)


def kkt(family, X, y, o, v, beta, lam, omega=None, b0=0.0):
    """-> (on, off, icpt): max |g_j - lam omega_j sign beta_j| over the support, max (|g_j| - lam omega_j) off it (-inf when
    empty) and |sum v (y - mu)| / n, with g = X'(v (y - mu)) / n."""
    n, p = X.shape
    om = np.ones(p) if omega is None else np.asarray(omega, dtype=np.float64)
    g = -gradient(family, X, y, o, v, beta, b0)
    eta = _lin(X, beta, b0) + (0.0 if (o is None or family == "binomial") else o)
    nz = beta != 0.0
    on = float(np.max(np.abs(g[nz] - lam * om[nz] * np.sign(beta[nz])))) if nz.any() else 0.0
    off = float(np.max(np.abs(g[~nz]) - lam * om[~nz])) if (~nz).any() else -np.inf
    return on, off, float(abs(np.sum(v * (y - mean(family, eta)))) / n)


def glm_path(family, X, y, o, v, lams, standardize=True, options=None, optTol=1e-7, intercept=False):
    """The warm-started path, omega the UNWEIGHTED column rms: -> list of (beta, b0, rounds, converged, rise)."""
    n, p = X.shape
    om = np.sqrt((X * X).sum(axis=0) / n) if standardize else np.ones(p)
    out, warm = [], None
    for lam in lams:
        b, b0, rounds, conv, rise = glm_lasso(family, X, y, o, v, lam, om, options, optTol=optTol, beta0=warm, intercept=intercept)
        warm = np.r_[b, b0] if intercept else b
        out.append((b, b0, rounds, conv, rise))
    return out


# ---- cross-validation ----------------------------------------------------------------------------------------------------------
def fold_scale(v, held, standardize):
    """The factor on lambda with which the handle's problem over all n rows -- (1/n) sum_train v nll, omega = sqrt(sum_train
    x^2 / n) when standardising -- has the minimiser of the fresh weighted problem on the training rows at lambda:
    (V_k / n) / sqrt(n_k / n), or V_k / n with omega = 1; V_k = sum_train v."""
    n, nk, vk = len(v), int((~held).sum()), float(np.sum(v[~held]))
    return (vk / n) / np.sqrt(nk / n) if standardize else vk / n


def subset(X, y, o, v, keep):
    """The fresh problem on the rows `keep`: their weights renormalised to sum to their number."""
    return np.asfortranarray(X[keep]), y[keep], (None if o is None else o[keep]), normalise(v[keep])


def masked_lasso(family, X, y, o, v, held, lam, standardize=True, optTol=1e-7, intercept=False, maxIter=25):
    """The product's route on the oracle's CDWeightedLSLoss over ALL n rows: the weighted rows, then w = 0 and z = eta_lin on
    the held-out rows, omega = sqrt(sum_train x^2 / n) (or ones; the intercept's 0), lambda fold_scale(); started at zero
    (the intercept at the null model of the training rows).  -> (beta (length p), b0, rounds)."""
    n, p = X.shape
    X1 = LG.with_ones(X) if intercept else X
    om = np.sqrt((X[~held] ** 2).sum(axis=0) / n) if standardize else np.ones(p)
    om1 = np.r_[om, 0.0] if intercept else om
    beta = np.zeros(X1.shape[1])
    if intercept:
        beta[p] = null_intercept(family, y[~held], None if o is None else o[~held], v[~held])
    x = O.SparseIterate(X1.shape[1], beta)
    g = O.ProxL1(lam * fold_scale(v, held, standardize), om1)
    options = O.CDOptions(maxIter=100000, optTol=1e-12, randomize=False)
    rounds = 0
    for _ in range(maxIter):
        eta_lin = X1 @ beta
        o_ = rows(family, y, eta_lin, o, v)
        w, z = np.where(held, 0.0, o_["w"]), np.where(held, eta_lin, o_["z"])
        O.coordinateDescent_(x, O.CDWeightedLSLoss(z, X1, w), g, options)
        new = x.dense()
        rounds += 1
        step = float(np.max(np.abs(new - beta)))
        beta = new
        if step < optTol:
            break
    return beta[:p].copy(), float(beta[p]) if intercept else 0.0, rounds


def cv(family, X, y, o, v, lams, K, ids, intercept=False, standardize=True, optTol=1e-10):
    """Cross-validation by row subsetting -> dict(paths[k] = glm_path's list, fold_deviance = sum_held v dev / sum_held v,
    fold_class = sum_held v miss / sum_held v (binomial), train_deviance = sum_train v dev / V_k, weights = sum_held v, sizes,
    and per measure (cvm, cvsd, index_min, index_1se), the folds weighted by sum_held v)."""
    m = len(lams)
    dev, tdev, cls = np.zeros((K, m)), np.zeros((K, m)), np.zeros((K, m))
    paths = []
    for k in range(K):
        held = ids == k
        Xt, yt, ot, vt = subset(X, y, o, v, ~held)
        path = glm_path(family, Xt, yt, ot, vt, lams, standardize, optTol=optTol, intercept=intercept)
        paths.append(path)
        vh, vtr = v[held], v[~held]
        for j, (b, b0, _, _, _) in enumerate(path):
            eh, et = X[held] @ b + b0, X[~held] @ b + b0
            rh = rows(family, y[held], eh, None if o is None else o[held], vh, 1e-300, 700.0)
            rt = rows(family, y[~held], et, None if o is None else o[~held], vtr, 1e-300, 700.0)
            dev[k, j] = np.sum(vh * rh["dev"]) / np.sum(vh)
            tdev[k, j] = np.sum(vtr * rt["dev"]) / np.sum(vtr)
            cls[k, j] = np.sum(vh * CVL.miss(y[held], eh)) / np.sum(vh)
    wts = np.bincount(ids, weights=v, minlength=K)
    out = dict(paths=paths, fold_deviance=dev, train_deviance=tdev, fold_class=cls, weights=wts, sizes=np.bincount(ids, minlength=K))
    for measure, err in (("deviance", dev), ("class", cls)):
        cvm, cvsd = CV.cv_curve(wts, err)
        out[measure] = (cvm, cvsd) + CV.select(lams, cvm, cvsd)
    return out


# ---- data ----------------------------------------------------------------------------------------------------------------------
def weights(n, seed, lo=1e-3, hi=1e3):
    """Log-uniform weights over [lo, hi], normalised to sum to n."""
    rng = np.random.default_rng(1000 + seed)
    return normalise(np.exp(rng.uniform(np.log(lo), np.log(hi), n)))


def make_data(family, n, p, s, seed, spread=(0.25, 4.0)):
    """-> (X, y, o, v): the unweighted twins' generators and log-uniform weights over `spread`, normalised."""
    if family == "binomial":
        X, y, _ = LG.make_data(n, p, s, seed)
        o = None
    else:
        X, y, o, _ = PN.make_data(seed, n, p, s)
    return X, y, o, weights(n, seed, *spread)


def replicate(X, y, o, reps):
    """Every row i repeated reps[i] times: the data an integer weight stands for."""
    idx = np.repeat(np.arange(len(y)), reps)
    return np.asfortranarray(X[idx]), y[idx], (None if o is None else o[idx])
