"""The numpy twin of cdh_glm_cox_score (csrc/cox_score.hip): Schoenfeld residuals, score residuals and the information matrix of
a Cox model with Breslow ties, strata and weights, for the columns X it is given, in two INDEPENDENT halves.

Per row, e = exp(min(eta, eta_max)) WITHOUT the weight, v the weight, ev = v e, dv = v delta, xt = x - centre, everything inside
the row's stratum.  For an event i whose risk set R_i = {j: t_j >= t_i} has S_i = sum ev > 0 (an event that counts):
    xbar_i = sum_R ev xt / S_i,     sch_i = xt_i - xbar_i (0 on every other row),     h_i = dv_i / S_i,
    L_i    = delta_i sch_i - e_i sum over the counting events k with t_k <= t_i of h_k (xt_i - xbar_k),
    I      = sum over the counting events of dv_i [sum_R ev xt xt' / S_i - xbar_i xbar_i'].

`definition` is the first half: explicit loops over the risk sets, found by comparing times, in long double -- no sort, no scan,
no position; O(n^2 m).  `scan` is the second half, line for line what the device does: the sort by (stratum, time) of
tests/_cox_strata_numpy.py, cumulative sums in LONG DOUBLE (unit roundoff 2^-64) that restart at the strata's bounds -- N the
suffix sums of ev xt, Q the prefix sums of h xbar, S and A the step's -- read at `first` and `last`, and I with the order of
summation swapped, sum ev A xt xt' - sum dv xbar xbar'.  It is the reference the GPU test holds the device to, and returns the
sizes that test's bounds are relative to: the same scans over the ABSOLUTE values.  tests/test_cox_score_host.py pins the halves
against each other.  xt is formed in float64, as the device forms it (one rounded subtraction), and ev and dv are the float64
products the kernels scan."""
import numpy as np

import _cox_numpy as CX
import _cox_strata_numpy as CS
from _cox_efron_numpy import _seg_cumsum

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a long double wider than float64"


def _inputs(X, eta_lin, off, status, eta_max, strata, weights, centre):
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    g = CS._ids(strata, n)
    v = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    mu = X.mean(axis=0) if centre is None else np.asarray(centre, dtype=np.float64)
    xt = X - mu                                                   # float64: the device's one rounded subtraction
    ec, e64, _ = CX.eta_of(eta_lin, off, eta_max)
    return xt, mu, g, v, e64, v * e64, v * np.asarray(status, dtype=np.float64)


# ---- the first half: the definition ------------------------------------------------------------------------------------------
def definition(X, eta_lin, off, time, status, eta_max=50.0, strata=None, weights=None, centre=None):
    """-> dict(sch, score: n x m long double; info: m x m long double; centre)."""
    xt64, mu, g, v, e64, ev64, dv64 = _inputs(X, eta_lin, off, status, eta_max, strata, weights, centre)
    time = np.asarray(time, dtype=np.float64)
    n, m = xt64.shape
    xt, e, ev, dv = xt64.astype(LD), e64.astype(LD), ev64.astype(LD), dv64.astype(LD)
    sch, L, info = np.zeros((n, m), dtype=LD), np.zeros((n, m), dtype=LD), np.zeros((m, m), dtype=LD)
    xbar, h = np.zeros((n, m), dtype=LD), np.zeros(n, dtype=LD)
    for i in range(n):
        if dv[i] == 0:
            continue
        risk = np.nonzero((g == g[i]) & (time >= time[i]))[0]
        S = ev[risk].sum()
        if not S > 0:
            continue
        h[i] = dv[i] / S
        xbar[i] = (ev[risk, None] * xt[risk]).sum(axis=0) / S
        sch[i] = xt[i] - xbar[i]
        second = (ev[risk, None, None] * xt[risk, :, None] * xt[risk, None, :]).sum(axis=0) / S
        info += dv[i] * (second - np.outer(xbar[i], xbar[i]))
    for i in range(n):
        acc = np.zeros(m, dtype=LD)
        for k in np.nonzero((g == g[i]) & (time <= time[i]) & (h != 0))[0]:
            acc += h[k] * (xt[i] - xbar[k])
        L[i] = (sch[i] if status[i] != 0 else 0) - e[i] * acc
    return dict(sch=sch, score=L, info=info, centre=mu)


# ---- the second half: the scans ----------------------------------------------------------------------------------------------
def scan(X, eta_lin, off, time, status, eta_max=50.0, strata=None, weights=None, centre=None, dtype=LD):
    """-> dict(sch, score, info, centre) and, per row and column unless said otherwise, what the GPU test's bounds are relative
    to: xt, e and A (per row), counts (per row: an event that counts), Xabs (sum ev |xt| / S of the row's tie group), Qabs (the
    prefix sums of h Xabs read where Q is read), I1abs and I2abs (m x m: the two sums of I over absolute values); order."""
    xt64, mu, g, v, e64, ev64, dv64 = _inputs(X, eta_lin, off, status, eta_max, strata, weights, centre)
    n, m = xt64.shape
    order, first, last, sfirst, slast = CS.groups(time, g)
    xs, es, evs, dvs = xt64[order].astype(dtype), e64[order].astype(dtype), ev64[order].astype(dtype), dv64[order].astype(dtype)
    T = _seg_cumsum(evs, sfirst, slast, reverse=True)
    S = T[first]
    counts = (dvs != 0) & (S > 0)
    Ssafe = np.where(S > 0, S, 1)
    h = np.where(counts, dvs / Ssafe, 0)
    A = _seg_cumsum(h, sfirst, slast)[last]
    sch, L = np.zeros((n, m), dtype=dtype), np.zeros((n, m), dtype=dtype)
    Xabs, Qabs, xbar_all = np.zeros((n, m), dtype=dtype), np.zeros((n, m), dtype=dtype), np.zeros((n, m), dtype=dtype)
    for c in range(m):
        x = xs[:, c]
        N = _seg_cumsum(evs * x, sfirst, slast, reverse=True)
        Na = _seg_cumsum(evs * np.abs(x), sfirst, slast, reverse=True)
        xbar = np.where(S > 0, N[first] / Ssafe, 0)
        xa = np.where(S > 0, Na[first] / Ssafe, 0)
        Q = _seg_cumsum(np.where(counts, h * xbar, 0), sfirst, slast)[last]
        Qa = _seg_cumsum(np.where(counts, h * xa, 0), sfirst, slast)[last]
        s_c = np.where(counts, x - xbar, 0)
        sch[order, c] = s_c
        L[order, c] = s_c - es * (x * A - Q)
        Xabs[order, c], Qabs[order, c], xbar_all[:, c] = xa, Qa, xbar
    wA = evs * A
    xb = np.where(counts[:, None], xbar_all, 0)
    dk = np.where(counts, dvs, 0)
    xa_sorted = np.where(counts[:, None], Xabs[order], 0)
    info = np.einsum("s,sc,sd->cd", wA, xs, xs) - np.einsum("s,sc,sd->cd", dk, xb, xb)
    I1abs = np.einsum("s,sc,sd->cd", wA, np.abs(xs), np.abs(xs))
    I2abs = np.einsum("s,sc,sd->cd", dk, xa_sorted, xa_sorted)
    back = lambda a: a[np.argsort(order)]
    return dict(sch=sch, score=L, info=info, centre=mu, xt=xt64, e=back(es), A=back(A), counts=back(counts), Xabs=Xabs, Qabs=Qabs,
                I1abs=I1abs, I2abs=I2abs, order=order, S=back(S), v=v, ev=back(evs), dv=back(dvs))


def inference(X, beta, eta_lin, off, time, status, strata=None, weights=None, cluster=None, eta_max=50.0):
    """var = I^-1, se, z, and the robust pieces of R's coxph(robust = TRUE): dfbeta = diag(v) L I^-1, summed over cluster ids when
    given, robust_var = D'D -- from the definition half, in long double, solved in float64."""
    q = definition(X, eta_lin, off, time, status, eta_max, strata, weights)
    info = q["info"].astype(np.float64)
    var = np.linalg.inv(info)
    v = np.ones(len(time)) if weights is None else np.asarray(weights, dtype=np.float64)
    dfbeta = (v[:, None] * q["score"].astype(np.float64)) @ var
    D = dfbeta
    if cluster is not None:
        ids = np.unique(cluster)
        D = np.stack([dfbeta[np.asarray(cluster) == i].sum(axis=0) for i in ids])
    rv = D.T @ D
    se = np.sqrt(np.diag(var))
    return dict(var=var, se=se, z=np.asarray(beta) / se, dfbeta=dfbeta, robust_var=rv, robust_se=np.sqrt(np.diag(rv)), info=info)
