"""The Cox model's post-estimation exports on the device: cdh_glm_cox_residuals and cdh_glm_cox_baseline (csrc/cox_post.hip, over
the scratch of the handle's own read-only step), held to the numpy twin's scan half in long double (tests/_cox_post_numpy.py;
its halves are pinned in tests/test_cox_post_host.py) at the eta the handle held, for the four chains -- plain, strata with
weights, start-stop times, Efron ties -- with rows in random order and pre-sorted.

The bounds are the sibling step tests', taken from their docstrings without change.  U = 2^-53, the twin's long-double values
taken as exact (their own error is 2^-11 of these bounds); rho and the sizes Ssz = T + T2 and Asz = P(stop) + P(start) are the
twin's, per stratum; everything is relative to the row's OWN stratum.
    A (cumhaz)        tests/test_gpu_cox_strata.py:    |dA| <= (2n + 18) U A                            plain and strata
                      tests/test_gpu_cox_interval.py:  |dA| <= cA U Asz,  cA = (n + 11) rho + n + 9      start-stop
                      tests/test_gpu_cox_efron.py:     |dA| <= (4n + 16) U rho A                        Efron
    S (risk_sum)      |dS| <= (n + 10) U S  (strata, Efron: S is the same scan),  (n + 11) U Ssz  (start-stop).
    table cumhaz      the stratum's prefix sum P_A itself, before any difference: the A bound with Asz = A for the censored
                      chains; ((n + 11) rho + n + 8) U P_A with start-stop times (the interval test's P_A line).
    table cumvar      the prefix sum P_B of the terms h2 = (dv / S) / S.  Censored chains: the strata test's |dB| <= (3n + 20) U B;
                      Efron: that test's (6n + 30) U rho B.  Start-stop times, derived as the interval test derives P_A: a term
                      carries S's relative error twice, 2 (n + 11) U rho = (2n + 22) U rho; the two divisions round once each
                      and the twin's S is rounded once, 2 U + U; dv = v delta is exact; the prefix scan adds at most n
                      positive terms, n U; first order in U, and 5 U of slack as in the P_A line's n + 8:
                          |dP_B| <= ((2n + 22) rho + n + 8) U P_B.
                      (The interval test's cB = (2n + 22) rho + n + 1 is the same count for the DIFFERENCE B, relative to
                      Bsz; the table holds P_B before any difference.)
    table n_event     a sum of at most n products v delta, each exact (delta is 0 or 1):  n U n_event; EXACT, compared with ==,
                      under unit weights.
    martingale        M = delta - e A is the step's d = dv - ev A without the factor v, which is one exact-to-U factor of both
                      terms: the siblings' |dd| bound divided by v,
                          bM = (2n + 68) U (delta + eA),   e cA U Asz + 50 U (delta + eA),   (4n + 66) U rho (delta + eA).
    deviance          compared through its square, dev2 = -2 (M + delta log(eA)), because the sum cancels where eA is near 1 and
                      no bound relative to dev2 itself can hold there.  M carries bM.  e A carries the same absolute error (delta
                      is exact and the subtraction rounds once, inside bM), so log(eA) carries bM / eA, and the library's log is
                      within an ulp: 2 U |log eA| with the twin's own.  The sum M + lg rounds once, U (|M| + |lg|); the factor
                      -2 is exact; the device's sqrt and this test's squaring add 3 U dev2 <= 6 U (|M| + |lg|):
                          |d dev2| <= 2 (bM + delta (bM / eA + 2 U |log eA|)) + 8 U (|M| + |log eA|).
                      A radicand that rounds below zero is taken as zero on the device and in the twin; an event with eA = 0 has
                      dev = +inf in both, compared with ==.  The sign is M's, compared with == wherever |M| exceeds bM.
Every case prints its rho and the worst measured multiple of each bound, which must be <= 1; LAB_NOTES.md "Cox lasso: baseline
hazard and residuals" holds the ones seen on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_plan as CP
import _cox_post_numpy as CPN
from test_gpu_cox import _step, _vp
from test_gpu_cox_efron import _group_sizes

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
T = CP.TILE
FULL = CP.MAX_GRID
WMIN, EMAX = 1e-5, 1.5
LD = np.longdouble

SIZES = [(1, FULL), (2, FULL), (65, FULL), (T + 1, FULL), (2 * T + 1, FULL), (5 * T + 3, 2)]
TIES = ("none", "one", "straddle")                             # one stratum
STRATA = ("strata", "noevent", "laststratum")                  # several strata, tie groups straddling every edge inside each
CHAINS = ("plain", "strata", "interval", "efron")
CASES = [(n, cap, pat, chain, presorted) for n, cap in SIZES for chain in CHAINS
         for pat in (TIES if chain == "plain" else TIES + STRATA) for presorted in (False, True)]
IDS = ["n%d-cap%d-%s-%s-%s" % (n, cap, pat, chain, "sorted-unit" if s else "random-weighted") for n, cap, pat, chain, s in CASES]

_DATA = {}


def _data(n, cap, pattern, chain, presorted):
    """X, start (or None), time, status, offset, strata ids (or None), weights (or None) and the iterate, built in SORTED layout
    and then dealt to the rows (the rows of one tie group keep their relative order: the sort is stable).  The plain chain has
    neither strata nor weights; the others carry random weights with rows in random order and none (unit) pre-sorted.  Computed
    once per case and left unchanged."""
    key = (n, cap, pattern, chain, presorted)
    if key in _DATA:
        return _DATA[key]
    rng = np.random.default_rng(4000 + n + 13 * (TIES + STRATA).index(pattern) + CHAINS.index(chain))
    g = np.zeros(n, dtype=np.int64)
    bounds = [0, n]
    if pattern in STRATA and n > 2:
        if pattern == "strata":                                  # the boundary inside a lane's four positions
            bounds = [0, 2 if n <= 65 else 4 * (n // 8) + 2, n]
        else:
            bounds = [0, n // 3, 2 * (n // 3), n]
        for i, (a, b) in enumerate(zip(bounds, bounds[1:])):
            g[a:b] = (0, 4, 9)[i] if len(bounds) == 4 else (0, 7)[i]
    if pattern == "none":
        sizes = [1] * n
    elif pattern == "one":
        sizes = [n]
    else:
        sizes = sum((_group_sizes(b - a, cap, a, n) for a, b in zip(bounds, bounds[1:])), [])
    assert sum(sizes) == n
    gid = np.repeat(np.arange(len(sizes)), sizes)
    first = np.r_[0, np.cumsum(sizes)[:-1]][gid]
    t = 1.0 + 0.5 * gid.astype(np.float64)
    if pattern == "strata" and n > 2:                            # the second stratum begins with the time the first ends with
        t[g == 7] = t[g == 7] - t[g == 7].min() + t[g == 0].max()
    status = (rng.random(n) < 0.7).astype(np.float64)
    if pattern == "noevent" and n > 2:
        status[g == 4] = 0.0
    if pattern == "laststratum" and n > 2:
        status[g != 9] = 0.0
    if not status.any():
        status[n - 1] = 1.0
    start = None
    if chain == "interval":                                      # starts on the grid of the times: they coincide with event times
        start = np.where(rng.random(n) < 0.3, 0.0, t - 0.5 * rng.integers(1, 5, n))
        assert np.all(start < t)
    X = np.asfortranarray(rng.standard_normal((n, 3)))
    off = rng.uniform(-0.5, 0.5, n)
    v = None if chain == "plain" or presorted else rng.uniform(0.25, 4.0, n)
    if not presorted:
        dest = rng.permutation(n)
        for a in np.unique(first):
            b = a + sizes[gid[a]]
            dest[a:b] = np.sort(dest[a:b])
        inv = np.argsort(dest)
        X, t, status, off, g = np.asfortranarray(X[inv]), t[inv], status[inv], off[inv], g[inv]
        v = None if v is None else v[inv]
        start = None if start is None else start[inv]
    gs = g if chain != "plain" and np.any(g != g[0]) else None
    x = cd.SparseIterate(3)
    x[1], x[2], x[3] = 0.8, -0.6, 0.4
    for a in (X, t, status, off, g) + tuple(b for b in (v, start) if b is not None):
        a.setflags(write=False)
    _DATA[key] = (X, start, t, status, off, gs, v, x)
    return _DATA[key]


def _loss(monkeypatch, chain, X, start, t, status, off, g, v, cap=FULL):
    if cap != FULL:
        monkeypatch.setenv("CDH_COX_GRID", str(cap))            # read when the handle is made
    y = np.c_[t, status] if start is None else np.c_[start, t, status]
    f = cd.CDCoxLoss(y, X, off, strata=g, weights=v)
    if chain == "efron":
        f.set_ties("efron")
    return f


def _residuals(f, eta_max=EMAX):
    out = [np.full(f.n, np.nan) for _ in range(3)]
    cd.check(f._L.cdh_glm_cox_residuals(f._h, float(eta_max), *[_vp(a) for a in out]), f._h)
    return dict(zip(("cumhaz", "martingale", "deviance"), out))


def _baseline(f, capacity, eta_max=EMAX):
    """-> (status, count, dict of columns cut to min(count, capacity))"""
    stratum = np.full(max(capacity, 1), -77, dtype=np.int32)
    cols = [np.full(max(capacity, 1), np.nan) for _ in range(5)]
    count = C.c_int64(-1)
    st = f._L.cdh_glm_cox_baseline(f._h, float(eta_max), int(capacity), _vp(stratum), *[_vp(c) for c in cols], C.byref(count))
    m = max(min(count.value, capacity), 0)
    tab = dict(zip(CPN.COLUMNS, [stratum[:m]] + [c[:m] for c in cols]))
    return st, count.value, tab


def _bounds(chain, n, q):
    """Per row: (the A bound, bM, the dev2 bound); per table row: dict of the four numeric columns' bounds."""
    rho, A, Asz, eA = q["rho"], np.abs(q["cumhaz"]).astype(np.float64), q["Asz"].astype(np.float64), q["eA"].astype(np.float64)
    e, delta = q["e"].astype(np.float64), q["delta"]
    tb = q["table"]
    trho = tb["rho"]
    f64 = lambda a: np.abs(np.asarray(a, dtype=np.float64))
    if chain == "interval":
        cA = (n + 11) * rho + n + 9
        bA = cA * U * Asz
        bM = e * cA * U * Asz + 50 * U * (delta + eA)
        bt = dict(n_event=n * U * f64(tb["n_event"]), risk_sum=(n + 11) * U * f64(tb["Ssz"]),
                  cumhaz=((n + 11) * trho + n + 8) * U * f64(tb["cumhaz"]), cumvar=((2 * n + 22) * trho + n + 8) * U * f64(tb["cumvar"]))
    elif chain == "efron":
        bA = (4 * n + 16) * U * rho * A
        bM = (4 * n + 66) * U * rho * (delta + eA)
        bt = dict(n_event=n * U * f64(tb["n_event"]), risk_sum=(n + 10) * U * f64(tb["risk_sum"]),
                  cumhaz=(4 * n + 16) * U * trho * f64(tb["cumhaz"]), cumvar=(6 * n + 30) * U * trho * f64(tb["cumvar"]))
    else:
        bA = (2 * n + 18) * U * A
        bM = (2 * n + 68) * U * (delta + eA)
        bt = dict(n_event=n * U * f64(tb["n_event"]), risk_sum=(n + 10) * U * f64(tb["risk_sum"]),
                  cumhaz=(2 * n + 18) * U * f64(tb["cumhaz"]), cumvar=(3 * n + 20) * U * f64(tb["cumvar"]))
    lg = f64(q["lg"])
    with np.errstate(divide="ignore", invalid="ignore"):
        b2 = 2 * (bM + np.where(delta != 0, bM / eA + 2 * U * lg, 0.0)) + 8 * U * (f64(q["martingale"]) + lg)
    return bA, bM, b2, bt


def _worst(err, bound):
    """The largest err / bound; an error where the bound is zero must be zero."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    z = bound == 0.0
    if np.any(err[z] != 0.0):
        return np.inf
    return float(np.max(err[~z] / bound[~z])) if np.any(~z) else 0.0


def _err(got, want):
    return np.abs(np.asarray(got, dtype=LD) - want).astype(np.float64)


# ---- both exports, case by case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,pattern,chain,presorted", CASES, ids=IDS)
def test_exports_row_by_row(monkeypatch, n, cap, pattern, chain, presorted):
    X, start, t, status, off, g, v, x = _data(n, cap, pattern, chain, presorted)
    tag = IDS[CASES.index((n, cap, pattern, chain, presorted))]
    f = _loss(monkeypatch, chain, X, start, t, status, off, g, v, cap)
    assert CP.padded(n) > n or n <= 2                            # pads exist
    cd.initialize_(f, x)
    y0, r0 = f.y, f.r
    eta_lin = y0 - r0
    vn = f.weights
    q = CPN.scan(eta_lin, off, t, status, EMAX, strata=g, weights=vn, start=start, ties="efron" if chain == "efron" else "breslow")
    rec0 = _step(f, -1, 0)                                       # the record of a read-only step without any post call
    res = _residuals(f)
    events = int(status.sum())
    st, count, tab = _baseline(f, events)
    assert st == OK
    # the table: which groups, in which order
    want = q["table"]
    assert count == len(want["time"]) and 1 <= count <= events
    assert np.array_equal(tab["stratum"], want["stratum"]) and np.array_equal(tab["time"], want["time"])
    assert np.all(np.lexsort((tab["time"], tab["stratum"])) == np.arange(count))
    if pattern == "none":
        assert count == events
    if pattern == "one":
        assert count == 1
    if pattern == "noevent" and n > 2:
        assert 4 not in tab["stratum"] and {0, 9} <= set(tab["stratum"].tolist())
    if pattern == "laststratum" and n > 2:
        assert set(tab["stratum"].tolist()) == {9}
    # the numbers, by the docstring's bounds
    bA, bM, b2, bt = _bounds(chain, n, q)
    m = {"A": _worst(_err(res["cumhaz"], q["cumhaz"]), bA), "M": _worst(_err(res["martingale"], q["martingale"]), bM)}
    fin = np.isfinite(q["dev2"].astype(np.float64))
    assert np.array_equal(np.isposinf(res["deviance"]), ~fin) and not np.any(np.isnan(res["deviance"]))
    m["dev2"] = _worst(_err(res["deviance"][fin].astype(LD) ** 2, q["dev2"][fin]), b2[fin])
    sure = np.abs(q["martingale"].astype(np.float64)) > bM
    assert np.array_equal(np.sign(res["deviance"][sure]), np.sign(q["martingale"][sure].astype(np.float64)))
    for key in ("n_event", "risk_sum", "cumhaz", "cumvar"):
        m[key] = _worst(_err(tab[key], want[key]), bt[key])
    if v is None:
        assert np.array_equal(tab["n_event"], want["n_event"].astype(np.float64))          # an event count, exactly
        assert np.all(tab["n_event"] == np.round(tab["n_event"])) and tab["n_event"].sum() == events
    print(f"cox post {tag}: rho {q['rho'].max():.3g}, table {count} of {events} events; worst multiples of the bounds: "
          + " ".join(f"{k} {val:.3f}" for k, val in m.items()))
    assert all(val <= 1.0 for val in m.values()), m
    # the invariant that does not go through the twin: sum of v M over a stratum is zero within the rows' own bounds
    ids = np.zeros(n, dtype=np.int64) if g is None else g
    for s in np.unique(ids):
        rows = ids == s
        total = CPN._lsum(vn[rows].astype(LD) * res["martingale"][rows].astype(LD))
        assert abs(total) <= float(np.sum(vn[rows] * bM[rows])) + n * U * float(np.sum(vn[rows] * (status[rows] + q["eA"][rows].astype(np.float64))))
    # purity: bit-identical on a second call; y and r are what they were; the step's record does not move
    res2 = _residuals(f)
    st2, count2, tab2 = _baseline(f, events)
    assert st2 == OK and count2 == count
    for k in res:
        assert np.array_equal(res[k], res2[k], equal_nan=True), k
    for k in tab:
        assert np.array_equal(tab[k], tab2[k]), k
    np.testing.assert_array_equal(f.y, y0)
    np.testing.assert_array_equal(f.r, r0)
    assert np.array_equal(_step(f, -1, 0), rec0)
    beta = np.zeros(f.p)
    cd.check(f._L.cdh_get_beta(f._h, _vp(beta)), f._h)
    np.testing.assert_array_equal(beta, x.dense())
    # a single output, and the others NULL: the same bits
    only = np.full(n, np.nan)
    cd.check(f._L.cdh_glm_cox_residuals(f._h, EMAX, None, _vp(only), None), f._h)
    np.testing.assert_array_equal(only, res["martingale"])
    # the step relation: v M is the d of a following applied step, r w on the rows it did not clamp
    out = _step(f, -1, 1)
    assert np.array_equal(out, rec0)
    w, z, r = f.w, f.y, f.r
    unc = w > WMIN
    rel = _worst(np.abs(vn * res["martingale"] - r * w)[unc], (2 * vn * bM + 2 * U * np.abs(r * w))[unc])
    print(f"cox post {tag}: v M against r w of the applied step on {int(unc.sum())} unclamped rows: {rel:.3f} of the bound")
    assert rel <= 1.0
    # and after the applied step the exports leave w, y and r alone as well
    _residuals(f)
    _baseline(f, events)
    for a, b in ((f.w, w), (f.y, z), (f.r, r)):
        np.testing.assert_array_equal(a, b)
    f.close()


def _lookup(tab, strata, times):
    """Per query (stratum, time): the index of the table row of that stratum with the largest time <= the query's, -1 if none;
    and whether that row's time IS the query's."""
    idx, exact = np.full(len(times), -1), np.zeros(len(times), dtype=bool)
    for s in np.unique(strata):
        rows = np.nonzero(tab["stratum"] == s)[0]
        sel = strata == s
        if len(rows) == 0:
            continue
        at = np.searchsorted(tab["time"][rows], times[sel], side="right") - 1
        idx[sel] = np.where(at >= 0, rows[np.maximum(at, 0)], -1)
        exact[sel] = (at >= 0) & (tab["time"][rows][np.maximum(at, 0)] == times[sel])
    return idx, exact


TWO = [(c, i) for c, i in zip(CASES, IDS) if c[2] in ("straddle", "noevent") and c[0] in (65, 2 * T + 1, 5 * T + 3)]
_TWO = {}


def _two_exports(monkeypatch, n, cap, pattern, chain, presorted):
    """Both exports of one handle, and per row the table's step function read at the row's time (less that read at its start,
    by cox_less's one rounded subtraction): -> (the rows the statement is about, cumhaz, the table's value, whether it was read
    in the row's OWN tie group and nothing was subtracted).  Run once per case, shared by the two tests below."""
    key = (n, cap, pattern, chain, presorted)
    if key not in _TWO:
        X, start, t, status, off, g, v, x = _data(n, cap, pattern, chain, presorted)
        f = _loss(monkeypatch, chain, X, start, t, status, off, g, v, cap)
        cd.initialize_(f, x)
        res = _residuals(f)
        st, count, tab = _baseline(f, int(status.sum()))
        assert st == OK
        f.close()
        ids = np.zeros(n, dtype=np.int64) if g is None else g
        H = np.r_[tab["cumhaz"], 0.0]                            # index -1: nothing yet
        at, exact = _lookup(tab, ids, t)
        want, own = H[at], exact
        if start is not None:                                    # cox_less: one rounded subtraction, nothing subtracted at -1
            en, _ = _lookup(tab, ids, start)
            want = np.where(en >= 0, H[at] - H[en], H[at])
            own = exact & (en < 0)
        rows = status == 0.0 if chain == "efron" else np.ones(n, dtype=bool)      # an Efron event reads its own expression
        _TWO[key] = (rows, res["cumhaz"], want, own)
    return _TWO[key]


@pytest.mark.parametrize("n,cap,pattern,chain,presorted", [c for c, _ in TWO], ids=[i for _, i in TWO])
def test_the_two_exports_agree_inside_a_tie_group(monkeypatch, n, cap, pattern, chain, presorted):
    """A row whose own (stratum, time) group is in the table holds that table row's cumhaz: the same stored double, ==."""
    rows, cumhaz, want, own = _two_exports(monkeypatch, n, cap, pattern, chain, presorted)
    assert n < 65 or (rows & own).sum() >= n // 8
    np.testing.assert_array_equal(cumhaz[rows & own], want[rows & own])


@pytest.mark.parametrize("n,cap,pattern,chain,presorted", [c for c, _ in TWO], ids=[i for _, i in TWO])
def test_the_two_exports_agree(monkeypatch, n, cap, pattern, chain, presorted):
    """Every row's cumhaz is the table's step function read at its time -- its own group's cumhaz, or the last earlier event
    group's of its stratum, or 0 -- and with start-stop times the same cox_less expression formed from the table: with ==.

    This holds because k_post_rows reads hA at the table's positions (csrc/cox_post.hip, post_at).  Read at last[s] and
    enter[s] themselves, as the step's apply kernels read it, it did NOT hold on an MI355X for rows whose own group holds no
    event: 2 to 25 rows per case at n = 2 T + 1 and 5 T + 3 differed from the table by up to 2.8 U (up to 177 U of the difference
    with start-stop times, and a few ulps of hA where the table's two entries are one) -- between the two positions k_cox_scan
    adds zeros only, but along another association of the same terms.  (tests/test_gpu_cox_interval.py's docstring says the
    same of hA[last] - hA[enter] where no event lies between.)"""
    rows, cumhaz, want, own = _two_exports(monkeypatch, n, cap, pattern, chain, presorted)
    differ = rows & (cumhaz != want)
    rel = np.abs(cumhaz - want)[rows] / np.where(want[rows] != 0.0, np.abs(want[rows]), np.inf)
    print(f"cox post two exports {chain} n={n}: {int(differ.sum())} of {int(rows.sum())} rows differ from the table's step function; "
          f"{int((differ & own).sum())} of them in a group the table holds; worst {float(rel.max()) / U:.2f} U; "
          f"{int((differ & (want == 0.0)).sum())} rows hold a nonzero where the table's difference is 0")
    assert not np.any(differ)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    X, start, t, status, off, g, v, x = _data(65, FULL, "straddle", "strata", False)
    f = _loss(monkeypatch, "strata", X, start, t, status, off, g, v)
    L, h = f._L, f._h
    cd.initialize_(f, x)
    y0, r0 = f.y, f.r
    err = lambda: L.cdh_last_error(h).decode()
    st, count, tab = _baseline(f, 65)
    assert st == OK and count > 1
    st, short, _ = _baseline(f, count - 1)
    assert st == BAD and short == count                          # count is written all the same
    assert str(count) in err() and str(count - 1) in err() and "capacity" in err()
    st, c0, _ = _baseline(f, 0)
    assert st == BAD and c0 == count
    cnt = C.c_int64(-5)
    assert L.cdh_glm_cox_baseline(h, EMAX, -1, None, None, None, None, None, None, C.byref(cnt)) == BAD and "capacity is negative" in err()
    assert cnt.value == -5
    assert L.cdh_glm_cox_baseline(h, EMAX, 65, None, None, None, None, None, None, None) == BAD and "count is NULL" in err()
    assert L.cdh_glm_cox_baseline(h, EMAX, 65, None, None, None, None, None, None, C.byref(cnt)) == OK and cnt.value == count
    a = np.zeros(65)
    for bad in (0.0, -1.0, 700.5, float("nan"), float("inf")):
        assert L.cdh_glm_cox_residuals(h, bad, _vp(a), None, None) == BAD and "eta_max" in err()
        assert L.cdh_glm_cox_baseline(h, bad, 65, None, None, None, None, None, None, C.byref(cnt)) == BAD and "eta_max" in err()
    assert L.cdh_glm_cox_residuals(h, EMAX, None, None, None) == BAD and "all NULL" in err()
    np.testing.assert_array_equal(f.y, y0)
    np.testing.assert_array_equal(f.r, r0)
    f.close()
    # a binomial handle, and a handle before any observations
    b = cd.CDLogisticLoss((status > 0).astype(np.float64), X)
    assert b._L.cdh_glm_cox_residuals(b._h, EMAX, _vp(a), None, None) == BAD
    assert "no survival data" in b._L.cdh_last_error(b._h).decode()
    assert b._L.cdh_glm_cox_baseline(b._h, EMAX, 65, None, None, None, None, None, None, C.byref(cnt)) == BAD
    assert "no survival data" in b._L.cdh_last_error(b._h).decode()
    b.close()
    w = cd.CDWeightedLSLoss(np.zeros(65), X, np.ones(65))
    assert w._L.cdh_glm_cox_residuals(w._h, EMAX, _vp(a), None, None) == BAD
    assert "no survival data" in w._L.cdh_last_error(w._h).decode()
    assert w._L.cdh_glm_cox_baseline(w._h, EMAX, 65, None, None, None, None, None, None, C.byref(cnt)) == BAD
    assert "no survival data" in w._L.cdh_last_error(w._h).decode()
    w.close()


# ---- the front ends ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", ("breslow", "efron"))
def test_front_ends_after_a_fit(ties):
    rng = np.random.default_rng(77)
    n, p = 300, 8
    X = np.asfortranarray(rng.standard_normal((n, p)))
    t = np.round(rng.exponential(1.0, n), 1) + 0.1
    status = (rng.random(n) < 0.7).astype(np.float64)
    g = 3 * rng.integers(0, 3, n) - 1
    v = rng.uniform(0.25, 4.0, n)
    off = rng.uniform(-0.3, 0.3, n)
    f = cd.CDCoxLoss(np.c_[t, status], X, off, strata=g, weights=v)
    f.set_ties(ties)
    lmax = cd.coxLambdaMax(f)
    sol = cd.coxLasso(f, None, 0.2 * lmax, ties=ties)
    beta = sol.x.dense()
    assert sol.converged and 1 <= sol.x.nnz < p
    eta_lin = f.y - f.r                                          # X beta as the handle holds it
    assert np.max(np.abs(eta_lin - X @ beta)) <= 1e-9
    q = CPN.scan(eta_lin, off, t, status, 50.0, strata=g, weights=f.weights, ties=ties)
    chain = "efron" if ties == "efron" else "strata"
    bA, bM, b2, bt = _bounds(chain, n, q)
    M = f.residuals()
    assert _worst(_err(M, q["martingale"]), bM) <= 1.0
    np.testing.assert_array_equal(cd.coxResiduals(f), M)
    np.testing.assert_array_equal(cd.coxResiduals(f, "martingale", 50.0), M)
    assert _worst(_err(f.residuals("cumhaz"), q["cumhaz"]), bA) <= 1.0
    dev = f.residuals(type="deviance")
    assert _worst(_err(dev.astype(LD) ** 2, q["dev2"]), b2) <= 1.0 and np.array_equal(np.sign(dev), np.sign(M))
    with pytest.raises(cd.ArgumentError, match="type must be"):
        f.residuals("schoenfeld")
    with pytest.raises(cd.ArgumentError, match="eta_max"):
        f.residuals(eta_max=0.0)
    base = f.baseline_hazard()
    assert isinstance(base, cd.CoxBaseline)
    want = q["table"]
    assert np.array_equal(base.stratum, want["stratum"]) and np.array_equal(base.time, want["time"]) and base.stratum.dtype == np.int32
    for key in ("n_event", "risk_sum", "cumhaz", "cumvar"):
        assert _worst(_err(getattr(base, key), want[key]), bt[key]) <= 1.0, key
    head = np.r_[True, base.stratum[1:] != base.stratum[:-1]]
    np.testing.assert_array_equal(base.hazard, np.where(head, base.cumhaz, base.cumhaz - np.r_[0.0, base.cumhaz[:-1]]))
    assert np.all(base.hazard > 0.0) and set(base.stratum.tolist()) == {-1, 2, 5}
    b2_ = cd.coxBaselineHazard(f)
    for k in cd.CoxBaseline.__dataclass_fields__:
        np.testing.assert_array_equal(getattr(base, k), getattr(b2_, k))
    # survival curves of five new rows
    Xn = rng.standard_normal((5, p))
    gn = np.array([-1, 2, 5, 5, -1])
    times = np.linspace(0.0, float(t.max()) + 1.0, 40)
    S = cd.coxSurvival(base, Xn @ beta, times, gn)
    assert S.shape == (5, 40) and np.all(np.diff(S, axis=1) <= 0.0) and np.all((S > 0.0) & (S <= 1.0)) and np.all(S[:, 0] == 1.0)
    np.testing.assert_allclose(S, CPN.survival(dict(stratum=base.stratum, time=base.time, cumhaz=base.cumhaz), Xn @ beta, times, gn),
                               rtol=1e-14)
    with pytest.raises(cd.ArgumentError, match="stratum 3 is not in the baseline table"):
        cd.coxSurvival(base, [0.0], times, [3])
    f.close()
