"""The numpy twin of the Cox step (csrc/cox_kernels.hpp), Breslow ties.  Two forms of the risk-set quantities

    S_i = sum of e_j over t_j >= t_i,   A_i = sum of delta_k / S_k and B_i = sum of delta_k / S_k^2 over t_k <= t_i:

`scans`, the O(n) form -- sort, cumulative sums in float64, read at the tie groups' bounds -- and `scans_exact`, the O(n^2)
definition written out with math.fsum (every sum correctly rounded).  `rows` then writes the kernel's own lines
(cox_eta, cox_row) over either.  A row outside `train` leaves the risk sets and the event sums (e = 0, delta = 0) and gets
w = 0, z = eta_lin, r = 0.  tests/test_cox_plan_host.py holds the two forms to each other and the gradient to a central
difference of `npl`; the GPU tests hold the device to `scans_exact`."""
import math

import numpy as np


def eta_of(eta_lin, off, eta_max):
    """cox_eta: (ec, e, capped)."""
    eta = eta_lin + (0.0 if off is None else off)
    capped = eta > eta_max
    ec = np.where(capped, eta_max, eta)
    return ec, np.exp(ec), capped


def groups(time):
    """order (stable ascending), and per SORTED position the first and last position of its tie group."""
    time = np.asarray(time, dtype=np.float64)
    n = len(time)
    order = np.argsort(time, kind="stable")
    ts = time[order]
    head = np.r_[True, ts[1:] != ts[:-1]]
    starts = np.nonzero(head)[0]
    gid = np.cumsum(head) - 1
    ends = np.r_[starts[1:], n] - 1
    return order, starts[gid], ends[gid]


def scans(e, delta, time):
    """The O(n) form: (S, A, B) per row, by cumulative sums in sorted order."""
    order, first, last = groups(time)
    es, ds = e[order], delta[order]
    T = np.cumsum(es[::-1])[::-1]
    Ss = T[first]
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where((ds != 0.0) & (Ss > 0.0), ds / Ss, 0.0)
        h2 = np.where((ds != 0.0) & (Ss > 0.0), h / Ss, 0.0)
    As, Bs = np.cumsum(h)[last], np.cumsum(h2)[last]
    S, A, B = np.empty_like(e), np.empty_like(e), np.empty_like(e)
    S[order], A[order], B[order] = Ss, As, Bs
    return S, A, B


def scans_exact(e, delta, time):
    """The definition, every sum by math.fsum: S over {t_j >= t_i}, A and B over {t_k <= t_i}.  One evaluation per
    distinct time."""
    time = np.asarray(time, dtype=np.float64)
    uniq, inv = np.unique(time, return_inverse=True)
    Su = np.array([math.fsum(e[time >= t]) for t in uniq])
    S = Su[inv]
    ev = (delta != 0.0) & (S > 0.0)
    h = np.zeros_like(e)
    h2 = np.zeros_like(e)
    h[ev] = delta[ev] / S[ev]
    h2[ev] = h[ev] / S[ev]
    Au = np.array([math.fsum(h[time <= t]) for t in uniq])
    Bu = np.array([math.fsum(h2[time <= t]) for t in uniq])
    return S, Au[inv], Bu[inv]


def rows(eta_lin, off, time, status, wmin, eta_max, train=None, exact=False):
    """cox_row over every row -> dict of w, z, r, nll (per-row terms delta (log S - ec)), d = delta - eA, eA, e, S, A, B,
    clamped, capped (bool per row) and delta (the training status)."""
    n = len(eta_lin)
    train = np.ones(n, dtype=bool) if train is None else np.asarray(train, dtype=bool)
    ec, e_all, capped = eta_of(eta_lin, off, eta_max)
    e = np.where(train, e_all, 0.0)
    delta = np.where(train, status, 0.0)
    S, A, B = (scans_exact if exact else scans)(e, delta, time)
    eA = e_all * A
    eB = e_all * B
    w_raw = eA - e_all * eB
    clamped = ~(w_raw >= wmin)
    w = np.where(clamped, wmin, w_raw)
    d = delta - eA
    r = d / w
    z = eta_lin + r
    with np.errstate(divide="ignore"):
        nll = np.where((delta != 0.0) & (S > 0.0), np.log(S) - ec, 0.0)
    out = dict(w=np.where(train, w, 0.0), z=np.where(train, z, eta_lin), r=np.where(train, r, 0.0), nll=nll, d=d, eA=eA, e=e,
               S=S, A=A, B=B, clamped=clamped & train, capped=capped, delta=delta, w_raw=w_raw)
    return out


def npl(eta, time, status):
    """The negative log partial likelihood -sum delta_i (eta_i - log S_i), by the definition."""
    e = np.exp(eta)
    S, _, _ = scans_exact(e, status, time)
    return -math.fsum(status * (eta - np.log(S)))


def gradient(X, eta_lin, off, time, status, train=None):
    """g = -X'(delta - eA) / n over the training rows (n: all rows, the handle's scaling), and eA."""
    q = rows(eta_lin, off, time, status, 1e-300, 700.0, train, exact=True)
    d = q["d"] if train is None else np.where(train, q["d"], 0.0)
    return -(X.T @ d) / len(eta_lin), q["eA"]


def make_data(n, p, seed, decimals=1, censor=0.3, presorted=False, with_offset=False):
    """A survival problem with ties: exponential times with hazard exp(X beta0), rounded to `decimals` (None: distinct),
    a fraction `censor` of the rows censored at random."""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    beta0 = np.zeros(p)
    beta0[: min(3, p)] = (0.8, -0.6, 0.4)[: min(3, p)]
    off = rng.uniform(-0.5, 0.5, n) if with_offset else None
    t = rng.exponential(1.0, n) / np.exp(X @ beta0 + (0.0 if off is None else off))
    if decimals is not None:
        t = np.round(t, decimals)
    status = (rng.random(n) >= censor).astype(np.float64)
    if not status.any():
        status[0] = 1.0
    if presorted:
        o = np.argsort(t, kind="stable")
        X, t, status = np.asfortranarray(X[o]), t[o], status[o]
        off = None if off is None else off[o]
    return X, t, status, off


def weighted_lasso(X, z, w, lam, omega, beta, optTol=1e-12, maxIter=10000):
    """Cyclic coordinate descent on (1/2n) sum w (z - X beta)^2 + lam sum omega |beta|, warm-started from beta (changed in
    place); stops when a full pass moves no coordinate by optTol or more."""
    n, p = X.shape
    r = z - X @ beta
    a = (X * X * w[:, None]).sum(axis=0) / n
    for _ in range(maxIter):
        worst = 0.0
        for j in range(p):
            if a[j] == 0.0:
                continue
            g = (X[:, j] * w) @ r / n + a[j] * beta[j]
            new = np.sign(g) * max(abs(g) - lam * omega[j], 0.0) / a[j]
            if new != beta[j]:
                r -= X[:, j] * (new - beta[j])
                worst = max(worst, abs(new - beta[j]))
                beta[j] = new
        if worst < optTol:
            break
    return beta


def cox_lasso(X, time, status, off, lam, omega=None, beta=None, wmin=1e-5, eta_max=50.0, maxIter=25, optTol=1e-7, train=None):
    """The IRLS loop of coxLasso_ on the host: -> (beta, rounds, converged)."""
    n, p = X.shape
    omega = np.ones(p) if omega is None else omega
    beta = np.zeros(p) if beta is None else beta.copy()
    rounds, converged = 0, False
    for _ in range(maxIter):
        q = rows(X @ beta, off, time, status, wmin, eta_max, train)
        old = beta.copy()
        weighted_lasso(X, q["z"], q["w"], lam, omega, beta)
        rounds += 1
        if np.max(np.abs(beta - old)) < optTol:
            converged = True
            break
    return beta, rounds, converged


def kkt(X, beta, off, time, status, lam, omega=None, train=None):
    """-> (worst violation off the support, worst on it, the scale max_j sum_k |X_j' diag(eA) X_k| / n of the KKT tolerance:
    eA dominates the Hessian of the partial likelihood, so the scale bounds what a unit move of beta does to the gradient)."""
    n, p = X.shape
    omega = np.ones(p) if omega is None else omega
    g, eA = gradient(X, X @ beta, off, time, status, train)
    if train is not None:
        eA = np.where(train, eA, 0.0)
    H = float(np.max(np.abs((X * eA[:, None]).T @ X).sum(axis=1))) / n
    on = beta != 0.0
    v_off = float(np.max(np.maximum(np.abs(g[~on]) - lam * omega[~on], 0.0))) if (~on).any() else 0.0
    v_on = float(np.max(np.abs(g[on] + lam * omega[on] * np.sign(beta[on])))) if on.any() else 0.0
    return v_off, v_on, H
