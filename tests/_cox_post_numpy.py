"""The numpy twin of the Cox model's post-estimation exports (csrc/cox_post.hip; cdh_glm_cox_residuals, cdh_glm_cox_baseline), in
two INDEPENDENT halves, for the four chains: plain, strata with weights, start-stop times, Efron ties.

Per row, e = exp(min(eta, eta_max)) WITHOUT the weight, v the weight, ev = v e, dv = v delta, everything inside the row's stratum:
    cumhaz_i     = A_i: the sum of the hazard increments of the event times the row was at risk at -- t <= t_i, or
                   start_i < t <= stop_i -- where the increment of a tie group g with risk-set sum S is (sum of dv over g) / S
                   under Breslow and sum_l m / den_l under Efron (m the group's mean event weight, den_l = S - (l / d) D), of
                   which an EVENT of g itself takes sum_l (1 - l / d) m / den_l;
    martingale_i = delta_i - e_i A_i;          deviance_i = sign(M_i) sqrt(max(0, -2 (M_i + delta_i log(e_i A_i)))).
The baseline table has one row per (stratum, time) that holds an event, in that order: n_event = sum of dv, risk_sum = S,
cumhaz and cumvar = the sums of the increments, and of increment / den (Breslow: n_event / S^2), up to and including that time.
An event group whose S (or den_l) is not > 0 adds nothing but keeps its row.

`definition` is the first half: O(n^2), risk sets by comparison of times, Efron by an explicit loop over l, every sum a
math.fsum of long doubles' worth -- no sort, no scan, no position.  `scan` is the second half, the form the device runs: the
sort by (stratum, time) of tests/_cox_strata_numpy.py, S from the sibling twins' exact rows (_cox_strata_numpy, _cox_interval_numpy,
_cox_efron_numpy in long double), and from there cumulative sums in LONG DOUBLE (unit roundoff 2^-64) that restart at the
strata's and the tie groups' bounds, read at `last`, `enter` and `first - 1` as the kernels read them.  It is the reference the
GPU tests hold the device to, and returns the sizes their bounds are relative to.  tests/test_cox_post_host.py pins the halves
against each other."""
import math

import numpy as np

import _cox_numpy as CX
import _cox_strata_numpy as CS
import _cox_interval_numpy as CI
import _cox_efron_numpy as CE

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a long double wider than float64"

COLUMNS = ("stratum", "time", "n_event", "risk_sum", "cumhaz", "cumvar")


def _lsum(x):
    """The sum of long doubles, by pairwise halves (error about log2(len) 2^-64: nothing beside the bounds' n 2^-53)."""
    x = np.asarray(x, dtype=LD)
    return LD(0) if len(x) == 0 else (x[0] if len(x) == 1 else _lsum(x[: len(x) // 2]) + _lsum(x[len(x) // 2:]))


def residual_lines(e, A, delta):
    """martingale, deviance and its square from e, A and delta, in long double: the kernel's lines."""
    e, A, delta = np.asarray(e, dtype=LD), np.asarray(A, dtype=LD), np.asarray(delta, dtype=LD)
    eA = e * A
    M = delta - eA
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.where(delta != 0, delta * np.log(np.where(delta != 0, eA, LD(1))), LD(0))
        rad = -2 * (M + lg)
    rad = np.where(rad < 0, LD(0), rad)
    return M, np.sign(M) * np.sqrt(rad), rad, eA, lg


# ---- the first half: the definition ------------------------------------------------------------------------------------------
def definition(eta_lin, off, stop, status, eta_max, strata=None, weights=None, start=None, ties="breslow"):
    """-> dict(cumhaz, martingale, deviance: long double per row; table: dict of COLUMNS).  O(n^2)."""
    stop = np.asarray(stop, dtype=np.float64)
    n = len(stop)
    g = CS._ids(strata, n)
    v = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    ec, _, _ = CX.eta_of(eta_lin, off, eta_max)
    e = np.exp(ec.astype(LD))
    ev = (v * np.exp(ec)).astype(LD)            # the kernels scan the float64 product of v and the float64 e
    dv = (v * status).astype(LD)
    enter = np.full(n, -np.inf) if start is None else np.asarray(start, dtype=np.float64)
    A = np.zeros(n, dtype=LD)
    table = []
    for s in np.unique(g):
        idx = np.nonzero(g == s)[0]
        events = idx[np.asarray(status)[idx] != 0]
        cum = cvar = LD(0)
        for t in np.unique(stop[events]):
            tied = events[stop[events] == t]
            atrisk = idx[(stop[idx] >= t) & (enter[idx] < t)]
            S, sdv, d = _lsum(ev[atrisk]), _lsum(dv[tied]), len(tied)
            inc = inc2 = own = LD(0)
            if ties == "efron":
                D, m = _lsum(ev[tied]), sdv / d
                for l in range(d):
                    den = S - (LD(l) / d) * D
                    if den > 0:
                        inc, inc2, own = inc + m / den, inc2 + m / den / den, own + (1 - LD(l) / d) * m / den
            elif S > 0:
                inc, inc2 = sdv / S, sdv / S / S
                own = inc
            cum, cvar = cum + inc, cvar + inc2
            table.append((int(s), t, sdv, S, cum, cvar))
            later = idx[(stop[idx] >= t) & (enter[idx] < t)]            # every row at risk at t accrues the increment ...
            A[later] += inc
            A[tied] += own - inc                                         # ... and an event of the group itself its own share
    M, dev, _, _, _ = residual_lines(e, A, status)
    cols = list(zip(*table))
    tab = {"stratum": np.asarray(cols[0], dtype=np.int32), "time": np.asarray(cols[1], dtype=np.float64)}
    for k, c in zip(COLUMNS[2:], cols[2:]):
        tab[k] = np.asarray(c, dtype=LD)
    return dict(cumhaz=A, martingale=M, deviance=dev, table=tab)


# ---- the second half: the scans ----------------------------------------------------------------------------------------------
def scan(eta_lin, off, stop, status, eta_max, strata=None, weights=None, start=None, ties="breslow"):
    """-> dict(cumhaz, martingale, deviance, dev2, eA, lg: long double per row; e, delta, v; table: dict of COLUMNS plus rho, Ssz
    per table row; and per row the sizes of the GPU tests' bounds: rho (the largest Ssz / S, or Efron's (S + frac D) / den, over
    the events of the row's stratum; 1 without a subtraction) and Asz (P(stop) + P(start); A itself without start times))."""
    stop = np.asarray(stop, dtype=np.float64)
    n = len(stop)
    g = CS._ids(strata, n)
    v = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    off0 = np.zeros(n) if off is None else off
    ec, e64, _ = CX.eta_of(eta_lin, off0, eta_max)
    ev, dv = v * e64, v * status
    seg = CE._seg_cumsum
    ratio = np.ones(n)                                            # per sorted position: what the subtraction in S or den costs
    if ties == "efron":
        assert start is None
        q, order = CE.scans(ev, dv, stop, g, LD)
        _, first, last, sfirst, slast = CS.groups(stop, g)
        enter = np.full(n, -1)
        Ss, ds = q["S"], dv[order].astype(LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            h = np.where(q["ok"], q["mm"] / q["den"], LD(0))
            h2 = np.where(q["ok"], h / q["den"], LD(0))
            ratio = np.where(q["ok"], (q["S"] + q["frac"] * q["D"]) / q["den"], 1).astype(np.float64)
        Ssz = Ss
    else:
        if start is None:
            order, first, last, sfirst, slast = CS.groups(stop, g)
            enter = np.full(n, -1)
            S = CS.rows(eta_lin, off0, stop, status, 1e-300, eta_max, exact=True, strata=g, weights=v)["S"]
            Ssz = S[order].astype(LD)
        else:
            order, first, last, sfirst, slast, _, _, enter = CI.groups(start, stop, g)
            S = CI.rows(eta_lin, off0, start, stop, status, 1e-300, eta_max, exact=True, strata=g, weights=v)["S"]
            Ssz = CI.rows(eta_lin, off0, start, stop, status, 1e-300, eta_max, strata=g, weights=v)["S_size"][order].astype(LD)
        Ss, ds = S[order].astype(LD), dv[order].astype(LD)
        haz = (ds != 0) & (Ss > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            h = np.where(haz, ds / np.where(haz, Ss, 1), LD(0))
            h2 = np.where(haz, h / np.where(haz, Ss, 1), LD(0))
            ratio = np.where(haz, Ssz / np.where(haz, Ss, 1), 1).astype(np.float64)
    cumA, cumB = seg(h, sfirst, slast), seg(h2, sfirst, slast)
    nev = seg(ds, first, last)
    sub = np.where(enter >= 0, cumA[np.maximum(enter, 0)], LD(0))
    A_sorted, Asz_sorted = cumA[last] - sub, cumA[last] + sub
    if ties == "efron":
        A_sorted = q["A"]
        Asz_sorted = A_sorted
    rho_sorted = np.ones(n)
    for a in np.unique(sfirst):
        m_ = sfirst == a
        rho_sorted[m_] = ratio[m_].max()
    A, Asz, rho = np.empty(n, dtype=LD), np.empty(n, dtype=LD), np.empty(n)
    A[order], Asz[order], rho[order] = A_sorted, Asz_sorted, rho_sorted
    e = np.exp(ec.astype(LD))
    M, dev, rad, eA, lg = residual_lines(e, A, status)
    flagged = (last == np.arange(n)) & (nev > 0)
    tab = dict(stratum=g[order][flagged].astype(np.int32), time=stop[order][flagged], n_event=nev[flagged],
               risk_sum=Ss[first][flagged], cumhaz=cumA[flagged], cumvar=cumB[flagged], rho=rho_sorted[flagged],
               Ssz=Ssz[first][flagged])
    return dict(cumhaz=A, martingale=M, deviance=dev, dev2=rad, eA=eA, lg=lg, e=e, delta=np.asarray(status, dtype=np.float64), v=v,
                rho=rho, Asz=Asz, table=tab, order=order, first=first, last=last, sfirst=sfirst, enter=enter)


def survival(tab, eta_new, times, strata_new):
    """exp(-H0_g(t) exp(eta)) by a loop over the rows and the times: H0 the largest cumhaz of the stratum at a time <= t."""
    out = np.empty((len(eta_new), len(times)))
    for i, (eta, s) in enumerate(zip(eta_new, strata_new)):
        for j, t in enumerate(times):
            hs = [float(c) for g, u, c in zip(tab["stratum"], tab["time"], tab["cumhaz"]) if g == s and u <= t]
            out[i, j] = math.exp(-(max(hs) if hs else 0.0) * math.exp(eta))
    return out
