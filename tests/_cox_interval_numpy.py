"""The numpy twin of the Cox step with start-stop times (csrc/cox_kernels.hpp, the interval chain), on top of
tests/_cox_strata_numpy.py.  Row i carries (start_i, stop_i], a weight v_i > 0 and a stratum id g_i, and is at risk at t iff
start_i < t <= stop_i; with ev = v e and dv = v delta, all inside the row's stratum,

    S(t) = sum of ev_j over stop_j >= t  -  sum of ev_j over start_j >= t,
    A_i  = P(stop_i) - P(start_i),  P(u) = sum of dv_k / S(stop_k) over the events k with stop_k <= u,  B_i likewise with dv / S^2.

`scans` is the O(n) difference form the device runs -- the (stratum, stop) order with its cumulative sums, a second order by
(stratum, start) with a second suffix sum T2, and the two lookups `lo` and `enter` of cox_order_interval (`groups`) -- and
`scans_exact` the definition: the explicit risk sets {start < t <= stop} per stratum, every sum by math.fsum and no
subtraction.  `rows` writes cox_row's lines over either (the lines of _cox_strata_numpy.rows).  start=None: every row is at
risk from -inf, and every function is _cox_strata_numpy's.  tests/test_cox_interval_plan_host.py holds the forms to each
other and to a central difference of `npl`; the GPU tests hold the device to `scans_exact`."""
import math

import numpy as np

import _cox_numpy as CX
import _cox_strata_numpy as CS


def groups(start, stop, strata=None):
    """-> (order, first, last, sfirst, slast, order2, lo, enter): the first five are _cox_strata_numpy.groups' on the stop times;
    order2 is the stable ascending order by (stratum, start); lo[s]: the first start-order position of s's stratum whose start
    is >= the stop time of stop-order position s, -1 if none; enter[s]: the last stop-order position of s's stratum whose stop is
    <= the start of row order[s], -1 if none."""
    start, stop = np.asarray(start, dtype=np.float64), np.asarray(stop, dtype=np.float64)
    n = len(stop)
    g = CS._ids(strata, n)
    order, first, last, sfirst, slast = CS.groups(stop, g)
    order2 = np.lexsort((start, g))
    lo, enter = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    for a, b in sorted(set(zip(sfirst.tolist(), slast.tolist()))):
        ts, ss = stop[order[a:b + 1]], start[order2[a:b + 1]]
        l = np.searchsorted(ss, ts, side="left")
        lo[a:b + 1] = np.where(l <= b - a, a + l, -1)
        e = np.searchsorted(ts, start[order[a:b + 1]], side="right") - 1
        enter[a:b + 1] = np.where(e >= 0, a + e, -1)
    return order, first, last, sfirst, slast, order2, lo, enter


def scans(ev, dv, start, stop, strata=None):
    """The O(n) difference form: (S, A, B, T + T2, P(stop) + P(start) of A, of B) per row; the last three are the sizes the
    rounding error of the three differences is relative to."""
    if start is None:
        S, A, B = CS.scans(ev, dv, stop, strata)
        return S, A, B, S, A, B
    order, first, last, sfirst, slast, order2, lo, enter = groups(start, stop, strata)
    es, ds, e2 = ev[order], dv[order], ev[order2]
    n = len(es)
    segs = sorted(set(zip(sfirst.tolist(), slast.tolist())))
    T, T2 = np.empty(n), np.empty(n)
    for a, b in segs:
        T[a:b + 1] = np.cumsum(es[a:b + 1][::-1])[::-1]
        T2[a:b + 1] = np.cumsum(e2[a:b + 1][::-1])[::-1]
    sub = np.where(lo >= 0, T2[np.maximum(lo, 0)], 0.0)
    Ss = T[first] - sub
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where((ds != 0.0) & (Ss > 0.0), ds / Ss, 0.0)
        h2 = np.where((ds != 0.0) & (Ss > 0.0), h / Ss, 0.0)
    cA, cB = np.empty(n), np.empty(n)
    for a, b in segs:
        cA[a:b + 1], cB[a:b + 1] = np.cumsum(h[a:b + 1]), np.cumsum(h2[a:b + 1])
    subA = np.where(enter >= 0, cA[np.maximum(enter, 0)], 0.0)
    subB = np.where(enter >= 0, cB[np.maximum(enter, 0)], 0.0)
    out = [np.empty_like(ev) for _ in range(6)]
    for o, v in zip(out, (Ss, cA[last] - subA, cB[last] - subB, T[first] + sub, cA[last] + subA, cB[last] + subB)):
        o[order] = v
    return tuple(out)


def scans_exact(ev, dv, start, stop, strata=None):
    """The definition: per stratum the risk set of t is {j: start_j < t <= stop_j}; S once per distinct stop time, A and B per
    row over the events with start_i < stop_k <= stop_i; every sum by math.fsum, no difference anywhere."""
    if start is None:
        return CS.scans_exact(ev, dv, stop, strata)
    start, stop = np.asarray(start, dtype=np.float64), np.asarray(stop, dtype=np.float64)
    g = CS._ids(strata, len(stop))
    S, A, B = np.zeros_like(ev), np.zeros_like(ev), np.zeros_like(ev)
    for s in np.unique(g):
        idx = np.nonzero(g == s)[0]
        a, b, e, d = start[idx], stop[idx], ev[idx], dv[idx]
        uniq, inv = np.unique(b, return_inverse=True)
        Ss = np.array([math.fsum(e[(a < t) & (b >= t)]) for t in uniq])[inv]
        haz = (d != 0.0) & (Ss > 0.0)
        h, h2 = np.zeros_like(e), np.zeros_like(e)
        h[haz] = d[haz] / Ss[haz]
        h2[haz] = h[haz] / Ss[haz]
        hb, h2b, bb = h[haz], h2[haz], b[haz]
        S[idx] = Ss
        A[idx] = [math.fsum(hb[(bb > a[i]) & (bb <= b[i])]) for i in range(len(idx))]
        B[idx] = [math.fsum(h2b[(bb > a[i]) & (bb <= b[i])]) for i in range(len(idx))]
    return S, A, B


def rows(eta_lin, off, start, stop, status, wmin, eta_max, train=None, exact=False, strata=None, weights=None):
    """The weighted, stratified cox_row over every row at risk on (start, stop] -> _cox_strata_numpy.rows' dict; the O(n) form
    adds S_size, A_size and B_size (scans)."""
    n = len(eta_lin)
    train = np.ones(n, dtype=bool) if train is None else np.asarray(train, dtype=bool)
    v = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    ec, e_all, capped = CX.eta_of(eta_lin, off, eta_max)
    ev_all = v * e_all
    ev = np.where(train, ev_all, 0.0)
    dv = np.where(train, v * status, 0.0)
    extra = {}
    if exact:
        S, A, B = scans_exact(ev, dv, start, stop, strata)
    else:
        S, A, B, extra["S_size"], extra["A_size"], extra["B_size"] = scans(ev, dv, start, stop, strata)
    evA = ev_all * A
    evB = ev_all * B
    w_raw = evA - ev_all * evB
    clamped = ~(w_raw >= wmin)
    w = np.where(clamped, wmin, w_raw)
    d = dv - evA
    r = d / w
    z = eta_lin + r
    with np.errstate(divide="ignore", invalid="ignore"):
        nll = dv * np.where((dv != 0.0) & (S > 0.0), np.log(np.where(S > 0.0, S, 1.0)) - ec, 0.0)
    return dict(w=np.where(train, w, 0.0), z=np.where(train, z, eta_lin), r=np.where(train, r, 0.0), nll=nll, d=d, eA=evA, e=ev,
                S=S, A=A, B=B, clamped=clamped & train, capped=capped, delta=dv, w_raw=w_raw, v=v, **extra)


def npl(eta, start, stop, status, strata=None, weights=None):
    """The negative log partial likelihood -sum dv_i (eta_i - log S_i), by the definition."""
    v = np.ones(len(eta)) if weights is None else np.asarray(weights, dtype=np.float64)
    dv = v * status
    S, _, _ = scans_exact(v * np.exp(eta), dv, start, stop, strata)
    ev = dv != 0.0
    return -math.fsum(dv[ev] * (eta[ev] - np.log(S[ev])))


def gradient(X, eta_lin, off, start, stop, status, train=None, strata=None, weights=None):
    """g = -X'(dv - evA) / n over the training rows (n: all rows, the handle's scaling), and evA."""
    q = rows(eta_lin, off, start, stop, status, 1e-300, 700.0, train, exact=True, strata=strata, weights=weights)
    d = q["d"] if train is None else np.where(train, q["d"], 0.0)
    return -(X.T @ d) / len(eta_lin), q["eA"]


def cox_lasso(X, start, stop, status, off, lam, omega=None, beta=None, wmin=1e-5, eta_max=50.0, maxIter=25, optTol=1e-7,
              train=None, strata=None, weights=None):
    """The IRLS loop of coxLasso_ on the host, with _cox_numpy.weighted_lasso per round: -> (beta, rounds, converged)."""
    n, p = X.shape
    omega = np.ones(p) if omega is None else omega
    beta = np.zeros(p) if beta is None else beta.copy()
    rounds, converged = 0, False
    for _ in range(maxIter):
        q = rows(X @ beta, off, start, stop, status, wmin, eta_max, train, strata=strata, weights=weights)
        old = beta.copy()
        CX.weighted_lasso(X, q["z"], q["w"], lam, omega, beta)
        rounds += 1
        if np.max(np.abs(beta - old)) < optTol:
            converged = True
            break
    return beta, rounds, converged


def kkt(X, beta, off, start, stop, status, lam, omega=None, train=None, strata=None, weights=None):
    """_cox_strata_numpy.kkt of the interval likelihood: -> (worst violation off the support, worst on it, the scale
    max_j sum_k |X_j' diag(evA) X_k| / n of the tolerance)."""
    n, p = X.shape
    omega = np.ones(p) if omega is None else omega
    g, evA = gradient(X, X @ beta, off, start, stop, status, train, strata, weights)
    if train is not None:
        evA = np.where(train, evA, 0.0)
    H = float(np.max(np.abs((X * evA[:, None]).T @ X).sum(axis=1))) / n
    on = beta != 0.0
    v_off = float(np.max(np.maximum(np.abs(g[~on]) - lam * omega[~on], 0.0))) if (~on).any() else 0.0
    v_on = float(np.max(np.abs(g[on] + lam * omega[on] * np.sign(beta[on])))) if on.any() else 0.0
    return v_off, v_on, H


BETA0 = (0.8, -0.6, 0.4)


def make_data(n, p, seed, rounded=False, zero=0.3, presorted=False):
    """The tests' start-stop problem: stop ~ Exp(1) + 0.05 (rounded: to one decimal, so that stops tie), start = stop U(0, 0.9),
    set to 0 with probability `zero` (rounded: floored to one decimal, which keeps start < stop and makes starts coincide with
    event times), status 1 with probability 0.7, an offset in +-0.5.  -> (X, start, stop, status, off); eta_lin = X @ beta0(p)."""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    off = rng.uniform(-0.5, 0.5, n)
    stop = rng.exponential(1.0, n) + 0.05
    if rounded:
        stop = np.round(stop, 1)
    start = stop * rng.uniform(0.0, 0.9, n)
    start = np.where(rng.random(n) < zero, 0.0, start)
    if rounded:
        start = np.floor(start * 10.0) / 10.0
    status = (rng.random(n) < 0.7).astype(np.float64)
    if not status.any():
        status[0] = 1.0
    if presorted:
        o = np.argsort(stop, kind="stable")
        X, start, stop, status, off = np.asfortranarray(X[o]), start[o], stop[o], status[o], off[o]
    assert np.all(start < stop)
    return X, start, stop, status, off


def beta0(p):
    b = np.zeros(p)
    b[: min(3, p)] = BETA0[: min(3, p)]
    return b


def split_rows(X, stop, status, off, cut):
    """Every row (0, t] with t > cut becomes (0, cut] censored plus (cut, t] with the same covariates: -> X, start, stop,
    status, off, and the index of the original row of every new one."""
    late = np.nonzero(stop > cut)[0]
    src = np.r_[np.arange(len(stop)), late]
    start = np.r_[np.zeros(len(stop)), np.full(len(late), cut)]
    stop2 = np.r_[np.where(stop > cut, cut, stop), stop[late]]
    status2 = np.r_[np.where(stop > cut, 0.0, status), status[late]]
    return np.asfortranarray(X[src]), start, stop2, status2, off[src], src
