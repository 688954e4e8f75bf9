"""The numpy twin of the Cox step with Efron ties (csrc/cox_efron.hip; cdh_glm_set_cox_ties), in two INDEPENDENT halves.

The first half, `npl`, is the negative log partial likelihood straight from the definition, a plain loop over the strata and
their distinct event times.  Per training row ev = v e and dv = v delta; a tie group g (one stratum, one time) has d events
among its training rows, D = sum of ev and m = (sum of dv) / d over them (survival::coxph's convention for weighted Efron) and
the risk-set sum S; den_l = S - (l / d) D for l = 0 .. d - 1, and

    n nll = sum_g [ m sum_l log den_l - sum over the events of g of dv eta ].

The second half, `rows`, is the step -- A, B, w, z, r and the record's terms -- written line for line as the kernels round:
the sort by (stratum, time), the event ranks and the group sums as cumulative sums that restart at the tie groups' bounds, the
four hazard terms per event, the cumulative hazards by stratum and by tie group, and cox_row's lines.  With dtype=np.float64
every operation is a float64 operation in the kernels' order of lines (the scans add in another order: cumsum is sequential);
with dtype=np.longdouble (x86's 80-bit format, unit roundoff 2^-64) the same lines serve as the reference the GPU tests hold
the device to: its own error is 2^-11 of any bound stated in multiples of n U.

    A_i = sum over the groups g at or before i's of m sum_l c / den_l,   B_i likewise with c^2 / den_l^2,
    c = 1 - l / d if i is an event of g itself, 1 otherwise (earlier groups, and the rows of g that are not events).

tests/test_cox_efron_host.py holds the two halves to each other by central differences, and to closed forms."""
import math

import numpy as np

import _cox_numpy as CX
import _cox_strata_numpy as CS

assert np.finfo(np.longdouble).nmant >= 63, "the reference needs a long double wider than float64"


# ---- the first half: the definition ------------------------------------------------------------------------------------------
def npl(eta, time, status, strata=None, weights=None, train=None):
    """n nll by the definition: a loop over the strata and their distinct event times, every sum by math.fsum."""
    eta = np.asarray(eta, dtype=np.float64)
    time = np.asarray(time, dtype=np.float64)
    n = len(eta)
    v = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    g = CS._ids(strata, n)
    tr = np.ones(n, dtype=bool) if train is None else np.asarray(train, dtype=bool)
    ev = v * np.exp(eta)
    total = []
    for s in np.unique(g[tr]):
        rows = np.nonzero(tr & (g == s))[0]
        events = rows[np.asarray(status)[rows] != 0]
        for t in np.unique(time[events]):
            tied = events[time[events] == t]
            d = len(tied)
            S = math.fsum(ev[rows[time[rows] >= t]])
            D = math.fsum(ev[tied])
            m = math.fsum(v[tied]) / d
            total.append(m * math.fsum(math.log(S - (l / d) * D) for l in range(d)))
            total.append(-math.fsum(v[tied] * eta[tied]))
    return math.fsum(total)


# ---- the second half: the step as the kernels write it -------------------------------------------------------------------------
def _seg_cumsum(x, lo, hi, reverse=False):
    """Cumulative sums of x that restart at every segment lo[s] .. hi[s] (suffix sums with reverse)."""
    out = np.empty_like(x)
    for a, b in sorted(set(zip(lo.tolist(), hi.tolist()))):
        seg = x[a:b + 1]
        out[a:b + 1] = np.cumsum(seg[::-1])[::-1] if reverse else np.cumsum(seg)
    return out


def scans(ev, dv, time, strata=None, dtype=np.float64):
    """ev, dv: per row, zero where the row is held out.  -> per SORTED position, in dtype: dict(A, B: the sums as the row at that
    position reads them; lg, mm: log den and m at an event that counts, else 0; S, den, frac, D, d, event) and `order`."""
    order, first, last, sfirst, slast = CS.groups(time, strata)
    es, ds = ev[order].astype(dtype), dv[order].astype(dtype)
    event = ds != 0
    one = event.astype(dtype)
    # k_efron_mark and the scans that follow it
    cnt = _seg_cumsum(one, first, last)
    Dv = _seg_cumsum(np.where(event, es, 0), first, last)
    Sdv = _seg_cumsum(ds, first, last, reverse=True)
    T = _seg_cumsum(es, sfirst, slast, reverse=True)
    # efron_term
    with np.errstate(divide="ignore", invalid="ignore"):
        d, D, sdv, S = cnt[last], Dv[last], Sdv[first], T[first]
        m = sdv / d
        frac = (cnt - 1) / d
        den = S - frac * D
        ok = event & (den > 0)
        cf = 1 - frac
        h = m / den
        h2 = h / den
        zero = np.zeros_like(es)
        hc = np.where(ok, cf * h, zero)
        hc2 = np.where(ok, (cf * cf) * h2, zero)
        lg = np.where(ok, np.log(np.where(ok, den, 1)), zero)
        h, h2, mm = np.where(ok, h, zero), np.where(ok, h2, zero), np.where(ok, m, zero)
    # the four scans, and what a row reads of them (k_efron_apply)
    hA, hB = _seg_cumsum(h, sfirst, slast), _seg_cumsum(h2, sfirst, slast)
    HC, HC2 = _seg_cumsum(hc, first, last), _seg_cumsum(hc2, first, last)
    some = first > sfirst
    before = np.maximum(first - 1, 0)
    A = np.where(event, np.where(some, hA[before], zero) + HC[last], hA[last])
    B = np.where(event, np.where(some, hB[before], zero) + HC2[last], hB[last])
    return dict(A=A, B=B, lg=lg, mm=mm, S=S, den=den, frac=frac, D=D, d=d, event=event, ok=ok, sfirst=sfirst), order


def rows(eta_lin, off, time, status, wmin, eta_max, train=None, strata=None, weights=None, dtype=np.float64):
    """The step over every row -> _cox_strata_numpy.rows' dict (e is ev, delta is dv, eA is ev A), in float64 whatever dtype the
    sums ran in, plus `rho`: per row, the largest (S + (l / d) D) / den over the training events of the row's stratum that
    count -- what the subtraction in den costs (1 where the stratum has none)."""
    n = len(eta_lin)
    train = np.ones(n, dtype=bool) if train is None else np.asarray(train, dtype=bool)
    v = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    off = np.zeros(n) if off is None else off
    ec, e_all, capped = CX.eta_of(eta_lin, off, eta_max)
    ev_all = v * e_all
    ev = np.where(train, ev_all, 0.0)
    dv = np.where(train, v * status, 0.0)
    q, order = scans(ev, dv, time, strata, dtype)
    A, B, mm, lg, S = (np.empty(n, dtype=dtype) for _ in range(5))
    A[order], B[order], mm[order], lg[order], S[order] = q["A"], q["B"], q["mm"], q["lg"], q["S"]
    evx, dvx = ev_all.astype(dtype), dv.astype(dtype)
    evA = evx * A
    evB = evx * B
    w_raw = evA - evx * evB
    clamped = ~(w_raw >= wmin)
    w = np.where(clamped, dtype(wmin), w_raw)
    d = dvx - evA
    r = d / w
    z = eta_lin.astype(dtype) + r
    nll = np.where(mm != 0, mm * lg - dvx * ec.astype(dtype), np.zeros(n, dtype=dtype))
    # rho, per stratum
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(q["ok"], (q["S"] + q["frac"] * q["D"]) / q["den"], 1).astype(np.float64)
    rho_sorted = np.ones(n)
    for a in np.unique(q["sfirst"]):
        m_ = q["sfirst"] == a
        rho_sorted[m_] = ratio[m_].max()
    rho = np.empty(n)
    rho[order] = rho_sorted
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    return dict(w=np.where(train, f64(w), 0.0), z=np.where(train, f64(z), eta_lin), r=np.where(train, f64(r), 0.0), nll=f64(nll),
                d=f64(d), eA=f64(evA), e=ev, S=f64(S), A=f64(A), B=f64(B), clamped=clamped & train, capped=capped, delta=dv,
                w_raw=f64(w_raw), v=v, rho=rho, lg=f64(lg), mm=f64(mm))


def gradient(X, eta_lin, off, time, status, train=None, strata=None, weights=None):
    """g = -X'(dv - ev A) / n over the training rows (n: all rows, the handle's scaling), and ev A."""
    q = rows(eta_lin, off, time, status, 1e-300, 700.0, train, strata, weights, dtype=np.longdouble)
    d = q["d"] if train is None else np.where(train, q["d"], 0.0)
    return -(X.T @ d) / len(eta_lin), q["eA"]


def kkt(X, beta, off, time, status, lam, omega=None, train=None, strata=None, weights=None):
    """_cox_strata_numpy.kkt with Efron's gradient: -> (worst violation off the support, worst on it, the tolerance's scale)."""
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
