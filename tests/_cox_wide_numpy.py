"""The wide twin of the Cox step: the O(n) forms of tests/_cox_numpy.py, tests/_cox_strata_numpy.py and
tests/_cox_interval_numpy.py with every cumulative sum, every division and every difference in np.longdouble (a 64-bit
mantissa: `scans` refuses to run where it is not), stratum by stratum, rounded to double ONCE at the end.  It is the reference
where the fsum definitions (`scans_exact`) cannot go -- they are quadratic in a stratum's rows -- and where the double O(n)
forms are no reference: their own error is of the size of the bound the device is held to.

With W = 2^-64: a cumulative sum of at most n positive terms is within n W of itself, so S (strata: the suffix sum T) is within
n W of the exact sum before its one rounding; a hazard term dv / S carries that and one division, the prefix sums n W more:
A and B are within (2n + 2) W and (3n + 3) W.  The interval form subtracts in longdouble, T - T2 and P(stop) - P(start): one
more W, relative to T + T2 and to P(stop) + P(start) as in the double form.  n W is 2^-11 of n U, U = 2^-53, whatever n is:
all of that stays below 2^-9 of the (n + 10) U, (2n + 18) U and (3n + 20) U the device is allowed, and the GPU tests use
their bounds unwidened.
tests/test_cox_wide_host.py holds this form to the fsum definitions at the shapes the other host tests use."""
import numpy as np

import _cox_interval_numpy as CI
import _cox_numpy as CX
import _cox_strata_numpy as CS

LD = np.longdouble


def scans(ev, dv, stop, strata=None, start=None):
    """(S, A, B, S_size, A_size, B_size) per row in double, from longdouble sums: S the sum of ev over the row's risk set, A and
    B the sums of dv / S and dv / S^2 over the events of its stratum inside its interval; the sizes are T + T2 and
    P(stop) + P(start), what the error of the interval form's differences is relative to (_cox_interval_numpy.scans' last
    three).  start=None: at risk from -inf, and the sizes are S, A and B."""
    assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than double here"
    ev, dv = np.asarray(ev, dtype=np.float64), np.asarray(dv, dtype=np.float64)
    n = len(ev)
    if start is None:
        order, first, last, sfirst, slast = CS.groups(stop, strata)
        lo = enter = None
    else:
        order, first, last, sfirst, slast, order2, lo, enter = CI.groups(start, stop, strata)
        e2 = ev[order2].astype(LD)
    es, ds = ev[order].astype(LD), dv[order].astype(LD)
    segs = sorted(set(zip(sfirst.tolist(), slast.tolist())))
    T = np.empty(n, dtype=LD)
    for a, b in segs:
        T[a:b + 1] = np.cumsum(es[a:b + 1][::-1])[::-1]
    Ss = Sz = T[first]
    if lo is not None:
        T2 = np.empty(n, dtype=LD)
        for a, b in segs:
            T2[a:b + 1] = np.cumsum(e2[a:b + 1][::-1])[::-1]
        sub = np.where(lo >= 0, T2[np.maximum(lo, 0)], LD(0))
        Ss, Sz = Ss - sub, Ss + sub
    haz = (ds != 0) & (Ss > 0)
    h = np.zeros(n, dtype=LD)
    h[haz] = ds[haz] / Ss[haz]
    h2 = np.zeros(n, dtype=LD)
    h2[haz] = h[haz] / Ss[haz]
    cA, cB = np.empty(n, dtype=LD), np.empty(n, dtype=LD)
    for a, b in segs:
        cA[a:b + 1], cB[a:b + 1] = np.cumsum(h[a:b + 1]), np.cumsum(h2[a:b + 1])
    As, Bs = Az, Bz = cA[last], cB[last]
    if enter is not None:
        subA = np.where(enter >= 0, cA[np.maximum(enter, 0)], LD(0))
        subB = np.where(enter >= 0, cB[np.maximum(enter, 0)], LD(0))
        As, Az, Bs, Bz = As - subA, As + subA, Bs - subB, Bs + subB
    out = [np.empty(n) for _ in range(6)]
    for o, x in zip(out, (Ss, As, Bs, Sz, Az, Bz)):
        o[order] = x.astype(np.float64)
    return tuple(out)


def rows(eta_lin, off, stop, status, wmin, eta_max, train=None, strata=None, weights=None, start=None):
    """cox_row's lines over the wide scans -> the dict of _cox_strata_numpy.rows (which is _cox_numpy.rows' where there are
    neither strata nor weights: v e and v delta are e and delta then, bit for bit), and the S_size, A_size and B_size of
    _cox_interval_numpy.rows' O(n) form."""
    n = len(eta_lin)
    train = np.ones(n, dtype=bool) if train is None else np.asarray(train, dtype=bool)
    v = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    ec, e_all, capped = CX.eta_of(eta_lin, off, eta_max)
    ev_all = v * e_all
    ev = np.where(train, ev_all, 0.0)
    dv = np.where(train, v * status, 0.0)
    S, A, B, S_size, A_size, B_size = scans(ev, dv, stop, strata, start)
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
                S=S, A=A, B=B, clamped=clamped & train, capped=capped, delta=dv, w_raw=w_raw, v=v, S_size=S_size, A_size=A_size,
                B_size=B_size)
