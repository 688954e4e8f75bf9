"""A numpy twin of the Poisson lasso: the IRLS loop over the CPU oracle's CDWeightedLSLoss / coordinateDescent_ (oracle/ is used,
not touched), written from the definitions and not from api.py.  The objective is
    F(beta) = (1/n) sum_i [mu_i - y_i eta_i] + lambda0 sum_j omega_j |beta_j|,   eta = X beta + o,  mu = exp(eta),
with counts y_i >= 0 and offsets o_i, and one round at the current beta forms, per row and in double,
    eta_lin = X beta;  eta = eta_lin + o;  capped = eta > eta_max, ec = min(eta, eta_max);  mu = exp(ec);
    clamped = mu < wmin, w = max(mu, wmin);  d = y - mu;  r = d / w;  z_lin = eta_lin + r;  nll = mu - y ec;
    dev = 2 ((y > 0 ? y log(y / mu) : 0) - (y - mu)),
then solves the weighted lasso on (z_lin, w) warm-started from beta: the offset is no part of the working response.  An
intercept is a trailing column of ones with omega = 0, started at log(sum y / sum exp(o)).

The cross-validation twin goes by ROW SUBSETTING -- the path of every fold is fitted on X[~held] alone and evaluated on
X[held] -- not by the 0/1 weights the product runs."""
import numpy as np

import oracle as O
import _cv_numpy as CV

U = 2.0 ** -53
WMIN, ETA_MAX = 1e-5, 50.0


def rows(y, eta_lin, o, wmin=WMIN, eta_max=ETA_MAX):
    """-> (w, z_lin, r, nll, dev, clamped, capped), each operation rounded on its own, in the order the kernel's pois_row takes
    them."""
    y, eta_lin = np.asarray(y, dtype=np.float64), np.asarray(eta_lin, dtype=np.float64)
    o = np.zeros_like(eta_lin) if o is None else np.asarray(o, dtype=np.float64)
    eta = eta_lin + o
    capped = eta > eta_max
    ec = np.where(capped, eta_max, eta)
    mu = np.exp(ec)
    clamped = mu < wmin
    w = np.where(clamped, wmin, mu)
    d = y - mu
    r = d / w
    z = eta_lin + r
    nll = mu - y * ec
    pos = y > 0.0
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        ylog = np.where(pos, y * np.log(np.where(pos, y, 1.0) / mu), 0.0)
    dev = 2.0 * (ylog - d)
    return w, z, r, nll, dev, clamped, capped


# seed -> (n, p, planted coefficients, intercept fitted?): the data sets of tests/test_poisson_host.py and tests/test_gpu_poisson.py
DATASETS = {0: (400, 30, 5, True), 1: (300, 60, 4, True), 2: (500, 20, 6, False)}
FRACS = (0.7, 0.4, 0.2, 0.1, 0.05)


def make_data(seed, n=None, p=None, s=None):
    """Gaussian X, the first s coefficients U(-.5, .5), o = log U(.5, 2), y ~ Poisson(exp(.3 + X beta* + o)); the generator is
    default_rng(seed), drawn in the order X, coefficients, exposures, counts.  -> (X, y, o, beta*)"""
    if n is None:
        n, p, s, _ = DATASETS[seed]
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    bstar = np.zeros(p)
    bstar[:s] = rng.uniform(-0.5, 0.5, s)
    o = np.log(rng.uniform(0.5, 2.0, n))
    y = rng.poisson(np.exp(0.3 + X @ bstar + o)).astype(np.float64)
    return X, y, o, bstar


def with_ones(X):
    return np.asfortranarray(np.hstack([X, np.ones((X.shape[0], 1))]))


def null_intercept(y, o=None):
    """The intercept of the null model: log(sum y / sum exp(o))."""
    return float(np.log(np.sum(y) / (len(y) if o is None else np.sum(np.exp(o)))))


def lambda_max(X, y, o=None, omega=None, intercept=False):
    """max_j |X_j'(y - mu)| / (n omega_j) at the null model: mu = exp(o), or exp(b0 + o) with the null intercept."""
    b0 = null_intercept(y, o) if intercept else 0.0
    mu = np.exp(b0 + (np.zeros(len(y)) if o is None else o))
    t = np.abs(X.T @ (y - mu)) / X.shape[0]
    return float(np.max(t if omega is None else t / omega))


def objective(X, y, o, beta, lam, omega=None, b0=0.0):
    nll = rows(y, X @ beta + b0, o)[3]
    om = np.ones(len(beta)) if omega is None else omega
    return float(np.mean(nll) + lam * np.sum(om * np.abs(beta)))


def poisson_lasso(X, y, o, lam, omega=None, options=None, maxIter=25, optTol=1e-7, wmin=WMIN, eta_max=ETA_MAX, beta0=None,
                  intercept=False):
    """-> (beta (length p), b0, rounds, converged, largest rise of F between two rounds).  beta0: warm start, length p (+ 1)."""
    n, p = X.shape
    X1 = with_ones(X) if intercept else X
    p1 = X1.shape[1]
    om = np.ones(p) if omega is None else np.asarray(omega, dtype=np.float64)
    om1 = np.r_[om, 0.0] if intercept else om
    options = options or O.CDOptions(maxIter=100000, optTol=1e-12, randomize=False)
    if beta0 is None:
        beta = np.zeros(p1)
        if intercept:
            beta[p] = null_intercept(y, o)
    else:
        beta = np.array(beta0, dtype=np.float64)
    x = O.SparseIterate(p1, beta)
    g = O.ProxL1(lam, om1)
    F = lambda b: float(np.mean(rows(y, X1 @ b, o, wmin, eta_max)[3]) + lam * np.sum(om1 * np.abs(b)))  # noqa: E731
    rise, Fprev, converged, rounds = -np.inf, F(beta), False, 0
    for _ in range(maxIter):
        w, z, _, _, _, _, _ = rows(y, X1 @ beta, o, wmin, eta_max)
        f = O.CDWeightedLSLoss(z, X1, w)
        O.coordinateDescent_(x, f, g, options)
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


def kkt(X, y, o, beta, lam, omega=None, b0=0.0):
    """-> (on, off, icpt): max |g_j - lam omega_j sign beta_j| over the support, max (|g_j| - lam omega_j) off it (-inf when
    empty) and |sum (y - mu)| / n, with g = X'(y - mu) / n at eta = X beta + b0 + o."""
    n, p = X.shape
    om = np.ones(p) if omega is None else np.asarray(omega, dtype=np.float64)
    res = y - np.exp(X @ beta + b0 + (0.0 if o is None else o))
    g = X.T @ res / n
    nz = beta != 0.0
    on = float(np.max(np.abs(g[nz] - lam * om[nz] * np.sign(beta[nz])))) if nz.any() else 0.0
    off = float(np.max(np.abs(g[~nz]) - lam * om[~nz])) if (~nz).any() else -np.inf
    return on, off, float(abs(np.sum(res)) / n)


def poisson_path(X, y, o, lams, standardize=True, options=None, optTol=1e-7, wmin=WMIN, eta_max=ETA_MAX, intercept=False):
    """The warm-started path: -> list of (beta, b0, rounds, converged, rise)."""
    n, p = X.shape
    om = np.sqrt((X * X).sum(axis=0) / n) if standardize else np.ones(p)
    out, warm = [], None
    for lam in lams:
        b, b0, rounds, conv, rise = poisson_lasso(X, y, o, lam, om, options, optTol=optTol, wmin=wmin, eta_max=eta_max,
                                                  beta0=warm, intercept=intercept)
        warm = np.r_[b, b0] if intercept else b
        out.append((b, b0, rounds, conv, rise))
    return out


def deviance(y, eta_lin, o=None):
    """The rows' Poisson deviances at the linear predictor eta_lin (+ o)."""
    return rows(y, eta_lin, o)[4]


def cv(X, y, o, lams, K, ids, intercept=False, standardize=True, optTol=1e-10):
    """Cross-validation by row subsetting -> dict(paths[k] = poisson_path's list, fold_deviance, train_deviance (means over the
    held-out and the training rows), sizes, cvm, cvsd, index_min, index_1se)."""
    m = len(lams)
    dev, tdev = np.zeros((K, m)), np.zeros((K, m))
    paths = []
    for k in range(K):
        held = ids == k
        Xt, yt, ot = np.asfortranarray(X[~held]), y[~held], (None if o is None else o[~held])
        Xh, yh, oh = X[held], y[held], (None if o is None else o[held])
        path = poisson_path(Xt, yt, ot, lams, standardize, optTol=optTol, intercept=intercept)
        paths.append(path)
        for j, (b, b0, _, _, _) in enumerate(path):
            dev[k, j] = np.mean(deviance(yh, Xh @ b + b0, oh))
            tdev[k, j] = np.mean(deviance(yt, Xt @ b + b0, ot))
    sizes = np.bincount(ids, minlength=K)
    cvm, cvsd = CV.cv_curve(sizes, dev)
    imin, i1se = CV.select(lams, cvm, cvsd)
    return dict(paths=paths, fold_deviance=dev, train_deviance=tdev, sizes=sizes, cvm=cvm, cvsd=cvsd, index_min=imin,
                index_1se=i1se)
