"""A numpy twin of the logistic lasso: the IRLS loop over the CPU oracle's CDWeightedLSLoss / coordinateDescent_ (oracle/ is used,
not touched), written from the definitions and not from api.py.  The objective is
    F(beta) = (1/n) sum_i [log(1 + e^eta_i) - y_i eta_i] + lambda0 sum_j omega_j |beta_j|,   eta = X beta,
and one round at the current beta forms, per row and in double,
    a = |eta|, e = exp(-a);  p = 1/(1+e) if eta >= 0 else e/(1+e), q = 1 - p taken from the other branch;
    w = max(e/(1+e)^2, wmin);  d = y q - (1-y) p;  r = d / w;  z = eta + r;  nll = max(eta, 0) + log1p(e) - y eta,
then solves the weighted lasso on (z, w) warm-started from beta.  An intercept is a trailing column of ones with omega = 0."""
import numpy as np

import oracle as O

U = 2.0 ** -53


def rows(y, eta, wmin):
    """-> (w, z, r, nll, clamped), each operation rounded on its own, in the order the kernel's glm_row takes them."""
    y, eta = np.asarray(y, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    a = np.abs(eta)
    e = np.exp(-a)
    ope = 1.0 + e
    big, small = 1.0 / ope, e / ope
    pos = eta >= 0.0
    p, q = np.where(pos, big, small), np.where(pos, small, big)
    w_raw = e / (ope * ope)
    clamped = w_raw < wmin
    w = np.where(clamped, wmin, w_raw)
    d = y * q - (1.0 - y) * p
    r = d / w
    z = eta + r
    nll = (np.maximum(eta, 0.0) + np.log1p(e)) - y * eta
    return w, z, r, nll, clamped


def prob(eta):
    e = np.exp(-np.abs(eta))
    return np.where(eta >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def make_data(n, p, s, seed, intercept=0.0):
    """Gaussian X, s coefficients of +-1 planted in the first s columns, y ~ Bernoulli(sigma(X beta* + intercept)); the
    generator is default_rng(seed), drawn in the order X, signs, uniforms."""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    bstar = np.zeros(p)
    bstar[:s] = rng.choice([-1.0, 1.0], s)
    u = rng.random(n)
    y = (u < prob(X @ bstar + intercept)).astype(np.float64)
    return X, y, bstar


def with_ones(X):
    return np.asfortranarray(np.hstack([X, np.ones((X.shape[0], 1))]))


def lambda_max(X, y, omega=None, intercept=False):
    """max_j |X_j'(y - p_hat)| / (n omega_j) at the null model (p_hat = 1/2, or the mean of y with an intercept)."""
    phat = np.mean(y) if intercept else 0.5
    t = np.abs(X.T @ (y - phat)) / X.shape[0]
    return float(np.max(t if omega is None else t / omega))


def objective(X, y, beta, lam, omega=None, b0=0.0):
    eta = X @ beta + b0
    nll = rows(y, eta, 0.25)[3]
    om = np.ones(len(beta)) if omega is None else omega
    return float(np.mean(nll) + lam * np.sum(om * np.abs(beta)))


def logistic_lasso(X, y, lam, omega=None, options=None, maxIter=25, optTol=1e-7, wmin=1e-5, beta0=None, intercept=False):
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
            ybar = np.mean(y)
            beta[p] = np.log(ybar / (1.0 - ybar))
    else:
        beta = np.array(beta0, dtype=np.float64)
    x = O.SparseIterate(p1, beta)
    g = O.ProxL1(lam, om1)
    F = lambda b: float(np.mean(rows(y, X1 @ b, 0.25)[3]) + lam * np.sum(om1 * np.abs(b)))  # noqa: E731
    rise, Fprev, converged, rounds = -np.inf, F(beta), False, 0
    for _ in range(maxIter):
        w, z, _, _, _ = rows(y, X1 @ beta, wmin)
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


def kkt(X, y, beta, lam, omega=None, b0=0.0):
    """-> (on, off, icpt): max |g_j - lam omega_j sign beta_j| over the support, max (|g_j| - lam omega_j) off it (-inf when
    empty) and |sum (y - p)| / n, with g = X'(y - p) / n at eta = X beta + b0."""
    n, p = X.shape
    om = np.ones(p) if omega is None else np.asarray(omega, dtype=np.float64)
    res = y - prob(X @ beta + b0)
    g = X.T @ res / n
    nz = beta != 0.0
    on = float(np.max(np.abs(g[nz] - lam * om[nz] * np.sign(beta[nz])))) if nz.any() else 0.0
    off = float(np.max(np.abs(g[~nz]) - lam * om[~nz])) if (~nz).any() else -np.inf
    return on, off, float(abs(np.sum(res)) / n)


def logistic_path(X, y, lams, standardize=True, options=None, optTol=1e-7, wmin=1e-5, intercept=False):
    """The warm-started path: -> list of (beta, b0, rounds)."""
    n, p = X.shape
    om = np.sqrt((X * X).sum(axis=0) / n) if standardize else np.ones(p)
    out, warm = [], None
    for lam in lams:
        b, b0, rounds, _, _ = logistic_lasso(X, y, lam, om, options, optTol=optTol, wmin=wmin, beta0=warm, intercept=intercept)
        warm = np.r_[b, b0] if intercept else b
        out.append((b, b0, rounds))
    return out
