"""The numpy twin of the Cox step with strata and observation weights (csrc/cox_kernels.hpp, the SW instantiations), on top of
tests/_cox_numpy.py.  Each row has a weight v_i > 0 and a stratum id g_i; with ev = v e and dv = v delta

    S_i = sum of ev_j over the rows j of g_i with t_j >= t_i,
    A_i = sum of dv_k / S_k and B_i = sum of dv_k / S_k^2 over the rows k of g_i with t_k <= t_i.

`scans` is the O(n) form -- a stable sort by (stratum, time), cumulative sums in float64 restarted at every stratum, read at
the tie groups' bounds -- and `scans_exact` the definition, stratum by stratum, every sum by math.fsum (_cox_numpy.scans_exact
on the stratum's rows).  `rows` writes the kernel's lines over either: ev = v e, evA = ev A, w_raw = evA - ev (ev B),
d = dv - evA, nll term dv (log S - ec).  tests/test_cox_strata_plan_host.py holds the forms to each other, to _cox_numpy and
to a central difference of `npl`; the GPU tests hold the device to `scans_exact`."""
import math

import numpy as np

import _cox_numpy as CX


def _ids(strata, n):
    return np.zeros(n, dtype=np.int64) if strata is None else np.asarray(strata).astype(np.int64)


def groups(time, strata=None):
    """order (stable ascending by (stratum, time)), and per SORTED position the first and last position of its tie group
    (same stratum and same time) and of its stratum: -> (order, first, last, sfirst, slast)."""
    time = np.asarray(time, dtype=np.float64)
    n = len(time)
    g = _ids(strata, n)
    order = np.lexsort((time, g))                                # the last key is the primary one; lexsort is stable
    ts, gs = time[order], g[order]
    shead = np.r_[True, gs[1:] != gs[:-1]]
    head = shead | np.r_[True, ts[1:] != ts[:-1]]

    def bounds(h):
        starts = np.nonzero(h)[0]
        gid = np.cumsum(h) - 1
        ends = np.r_[starts[1:], n] - 1
        return starts[gid], ends[gid]

    first, last = bounds(head)
    sfirst, slast = bounds(shead)
    return order, first, last, sfirst, slast


def scans(ev, dv, time, strata=None):
    """The O(n) form: (S, A, B) per row, by cumulative sums in sorted order that restart at every stratum."""
    order, first, last, sfirst, slast = groups(time, strata)
    es, ds = ev[order], dv[order]
    n = len(es)
    T = np.empty(n)
    for a, b in sorted(set(zip(sfirst.tolist(), slast.tolist()))):
        T[a:b + 1] = np.cumsum(es[a:b + 1][::-1])[::-1]
    Ss = T[first]
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where((ds != 0.0) & (Ss > 0.0), ds / Ss, 0.0)
        h2 = np.where((ds != 0.0) & (Ss > 0.0), h / Ss, 0.0)
    cA, cB = np.empty(n), np.empty(n)
    for a, b in sorted(set(zip(sfirst.tolist(), slast.tolist()))):
        cA[a:b + 1], cB[a:b + 1] = np.cumsum(h[a:b + 1]), np.cumsum(h2[a:b + 1])
    S, A, B = np.empty_like(ev), np.empty_like(ev), np.empty_like(ev)
    S[order], A[order], B[order] = Ss, cA[last], cB[last]
    return S, A, B


def scans_exact(ev, dv, time, strata=None):
    """The definition, stratum by stratum, every sum by math.fsum."""
    time = np.asarray(time, dtype=np.float64)
    g = _ids(strata, len(time))
    S, A, B = np.zeros_like(ev), np.zeros_like(ev), np.zeros_like(ev)
    for s in np.unique(g):
        m = g == s
        S[m], A[m], B[m] = CX.scans_exact(ev[m], dv[m], time[m])
    return S, A, B


def rows(eta_lin, off, time, status, wmin, eta_max, train=None, exact=False, strata=None, weights=None):
    """The weighted, stratified cox_row over every row -> _cox_numpy.rows' dict, in which e is ev, delta is dv and eA is evA;
    plus v."""
    n = len(eta_lin)
    train = np.ones(n, dtype=bool) if train is None else np.asarray(train, dtype=bool)
    v = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    ec, e_all, capped = CX.eta_of(eta_lin, off, eta_max)
    ev_all = v * e_all
    ev = np.where(train, ev_all, 0.0)
    dv = np.where(train, v * status, 0.0)
    S, A, B = (scans_exact if exact else scans)(ev, dv, time, strata)
    evA = ev_all * A
    evB = ev_all * B
    w_raw = evA - ev_all * evB
    clamped = ~(w_raw >= wmin)
    w = np.where(clamped, wmin, w_raw)
    d = dv - evA
    r = d / w
    z = eta_lin + r
    with np.errstate(divide="ignore"):
        nll = dv * np.where((dv != 0.0) & (S > 0.0), np.log(S) - ec, 0.0)
    return dict(w=np.where(train, w, 0.0), z=np.where(train, z, eta_lin), r=np.where(train, r, 0.0), nll=nll, d=d, eA=evA, e=ev,
                S=S, A=A, B=B, clamped=clamped & train, capped=capped, delta=dv, w_raw=w_raw, v=v)


def npl(eta, time, status, strata=None, weights=None):
    """The negative log partial likelihood -sum dv_i (eta_i - log S_i), by the definition."""
    v = np.ones(len(eta)) if weights is None else np.asarray(weights, dtype=np.float64)
    dv = v * status
    S, _, _ = scans_exact(v * np.exp(eta), dv, time, strata)
    return -math.fsum(dv * (eta - np.log(S)))


def gradient(X, eta_lin, off, time, status, train=None, strata=None, weights=None):
    """g = -X'(dv - evA) / n over the training rows (n: all rows, the handle's scaling), and evA."""
    q = rows(eta_lin, off, time, status, 1e-300, 700.0, train, exact=True, strata=strata, weights=weights)
    d = q["d"] if train is None else np.where(train, q["d"], 0.0)
    return -(X.T @ d) / len(eta_lin), q["eA"]


def cox_lasso(X, time, status, off, lam, omega=None, beta=None, wmin=1e-5, eta_max=50.0, maxIter=25, optTol=1e-7, train=None,
              strata=None, weights=None):
    """The IRLS loop of coxLasso_ on the host, with _cox_numpy.weighted_lasso per round: -> (beta, rounds, converged)."""
    n, p = X.shape
    omega = np.ones(p) if omega is None else omega
    beta = np.zeros(p) if beta is None else beta.copy()
    rounds, converged = 0, False
    for _ in range(maxIter):
        q = rows(X @ beta, off, time, status, wmin, eta_max, train, strata=strata, weights=weights)
        old = beta.copy()
        CX.weighted_lasso(X, q["z"], q["w"], lam, omega, beta)
        rounds += 1
        if np.max(np.abs(beta - old)) < optTol:
            converged = True
            break
    return beta, rounds, converged


def kkt(X, beta, off, time, status, lam, omega=None, train=None, strata=None, weights=None):
    """_cox_numpy.kkt of the weighted stratified partial likelihood: -> (worst violation off the support, worst on it, the
    scale max_j sum_k |X_j' diag(evA) X_k| / n of the tolerance)."""
    n, p = X.shape
    omega = np.ones(p) if omega is None else omega
    g, evA = gradient(X, X @ beta, off, time, status, train, strata, weights)
    if train is not None:
        evA = np.where(train, evA, 0.0)
    H = float(np.max(np.abs((X * evA[:, None]).T @ X).sum(axis=1))) / n
    on = beta != 0.0
    v_off = float(np.max(np.maximum(np.abs(g[~on]) - lam * omega[~on], 0.0))) if (~on).any() else 0.0
    v_on = float(np.max(np.abs(g[on] + lam * omega[on] * np.sign(beta[on])))) if on.any() else 0.0
    return v_off, v_on, H
