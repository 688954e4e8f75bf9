"""The Cox step with Efron ties on the device: cdh_glm_set_cox_ties, cdh_glm_get_cox_ties and cdh_glm_cox_irls over the chain of
csrc/cox_efron_host.hpp -- the tie-group scans and the three kernels of csrc/cox_efron.hip -- held row by row to the numpy twin
(tests/_cox_efron_numpy.py, its step half in long double; its halves are pinned in tests/test_cox_efron_host.py) at the eta the
handle held.

The bounds are tests/test_gpu_cox_strata.py's, line by line, with what Efron adds.  U = 2^-53, the twin's long-double values
taken as exact (their own error is 2^-11 of these bounds), d a group's events, everything relative to the row's OWN stratum:
    S                 as there:  |dS| <= (n + 10) U S.
    D                 a sum of at most d terms ev, each within 2 U:  |dD| <= (n + 2) U D.
    den = S - frac D  frac = l / d one rounding, frac D one more, the subtraction one more:
                      |d den| <= (n + 10) U S + (n + 4) U frac D + U den <= (n + 11) U (S + frac D) = (n + 11) U rho_l den,
                      rho_l = (S + frac D) / den.  This is the one subtraction Efron adds; D <= S gives rho_l <= 2 d.  A row's
                      bounds carry rho = the largest rho_l over the training events of the row's stratum (the twin's "rho").
    m = sdv / d       sdv a sum of at most d exact terms dv, one division:  (n + 1) U m.
    h = m / den       (n + 1) U + (n + 11) U rho + U  <=  (2n + 13) U rho h.
    c = 1 - frac      U frac from frac and U c from the subtraction; frac / c = l / (d - l) <= n:  (n + 1) U c.
    hc = c h          (n + 1) U + (2n + 13) U rho + U  <=  (3n + 15) U rho hc.
    A                 a scan of at most n positive terms, n U; a row that is an event adds two scans, one more U:
                      |dA| <= (4n + 16) U rho A                                        (there: (2n + 18) U A)
    h2, hc2, B        h2 = h / den: (3n + 25) U rho;  hc2 = (c c) h2: (2n + 4) U more, (5n + 29) U rho;  scan and the event
                      row's addition:  |dB| <= (6n + 30) U rho B                        (there: (3n + 20) U B)
    w (unclamped)     there A's and B's figures plus 38 U, relative to evA >= ev (ev B) -- which holds for Efron too, because a row's
                      share c ev of every den it enters is at most that den:  |dw| <= ((4n + 16) rho + (6n + 30) rho + 38) U evA
                      <= (10n + 84) U rho evA.
    d = dv - evA      there A's figure plus 50 U:  |dd| <= (4n + 66) U rho (dv + evA).
    r, z              as there:  |dr| <= (|dd| bound + |r| |dw| bound) / w,  |dz| <= |dr| bound + U |eta_lin|.
    sum w             (n + 64) U sum w, plus the rows' own |dw| bounds.
    sum dv            as there, and EXACT with unit weights.
    nll               an event's term is m lg - dv ec, lg = log den: the roundings of the two products, of the subtraction, m's
                      (n + 1) U and the sum's (n + 64) U, all relative to |m lg| + |dv ec|: (2n + 66) U of their sum; and the
                      logarithm's argument and its own rounding (the "floor" there): m ((n + 11) U rho_l + 2 U |lg|).
As in the sibling tests a clamp may differ from the twin only where the twin's w_raw is within the w bound of wmin; such rows
are left out of the w, r and z checks and counted.  Every case prints the worst measured multiple of its bounds and its
largest rho; LAB_NOTES.md "Cox lasso: Efron ties" holds the ones seen on an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_plan as CP
import _cox_efron_numpy as CE
import _cox_strata_numpy as CS
from test_gpu_cox import _pads_are_zero, _step, _vp

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
T = CP.TILE
FULL = CP.MAX_GRID
WMIN, EMAX = 1e-5, 1.5

SIZES = [(1, FULL), (2, FULL), (65, FULL), (T + 1, FULL), (2 * T + 1, FULL), (5 * T + 3, 2)]
PATTERNS = ("none", "one", "straddle", "first", "last", "alternating", "strata", "noevent")
CASES = [(n, cap, pat) for n, cap in SIZES for pat in PATTERNS]
IDS = ["n%d-cap%d-%s" % c for c in CASES]
COMBOS = [(wts, presorted) for wts in ("unit", "random") for presorted in (False, True)]


def _edges(n, cap):
    """The sorted positions a group should straddle: a wave's edge, a tile's edge, the edge between the capped grid's two runs."""
    pl = CP.plan(CP.padded(n), cap)
    e = {256, T}
    if pl["grid"] == 2:
        e.add(CP.run_first(pl["tiles"], 2, 1) * T)
    return sorted(b for b in e if 0 < b < n)


def _group_sizes(n, cap, lo=0, total=None):
    """Groups of 2 .. 7 cycling over positions lo .. lo + n - 1 of `total` (default: lo + n), none ending exactly on an edge of
    _edges unless the positions end there: each edge is straddled; with sizes that are no multiple of 4 the lanes' four
    positions are straddled all along."""
    edges, out, p, k = set(_edges(lo + n if total is None else total, cap)), [], lo, 0
    while p < lo + n:
        size = min(k % 6 + 2, lo + n - p)
        if p + size in edges and p + size < lo + n:
            size += 1 if size < 7 else -1
        out.append(size)
        p += size
        k += 1
    return out


_DATA = {}


def _data(n, cap, pattern, wts, presorted):
    """X, time, status, offset, strata ids, weights (None or uniform in [0.25, 4]) and the iterate, built in SORTED layout and then
    dealt to the rows: in random order the rows of one tie group keep their relative order (the sort is stable), so the events sit
    where the pattern puts them.  Computed once per case and left unchanged."""
    key = (n, cap, pattern, wts, presorted)
    if key in _DATA:
        return _DATA[key]
    rng = np.random.default_rng(3000 + n + 11 * PATTERNS.index(pattern))
    g = np.zeros(n, dtype=np.int64)
    if pattern == "none":
        sizes = [1] * n
    elif pattern == "one":
        sizes = [n]
    elif pattern == "strata" and n > 2:
        cut = 2 if n <= 65 else 4 * (n // 8) + 2                  # the boundary inside a lane's four positions
        g[cut:] = 7
        sizes = _group_sizes(cut, cap, 0, n) + _group_sizes(n - cut, cap, cut, n)
    elif pattern == "noevent" and n > 2:
        a, b = n // 3, 2 * (n // 3)
        g[a:b], g[b:] = 4, 9
        sizes = _group_sizes(a, cap, 0, n) + _group_sizes(b - a, cap, a, n) + _group_sizes(n - b, cap, b, n)
    else:
        sizes = _group_sizes(n, cap)
    assert sum(sizes) == n
    gid = np.repeat(np.arange(len(sizes)), sizes)
    first = np.r_[0, np.cumsum(sizes)[:-1]][gid]
    within = np.arange(n) - first
    size = np.asarray(sizes)[gid]
    t = 1.0 + 0.5 * gid.astype(np.float64)
    if pattern == "strata" and n > 2:
        # the second stratum begins with the time the first one ends with: two groups, not one
        t[g == 7] = t[g == 7] - t[g == 7].min() + t[g == 0].max()
    status = (rng.random(n) < 0.7).astype(np.float64)
    if pattern == "one":
        status[:] = 1.0
    elif pattern == "first":
        status = (within < (size + 1) // 2).astype(np.float64)
    elif pattern == "last":
        status = (within >= size // 2).astype(np.float64)
    elif pattern == "alternating":
        status = (within % 2 == 0).astype(np.float64)
    elif pattern == "noevent" and n > 2:
        status[g == 4] = 0.0
    if not status.any():
        status[0] = 1.0
    X = np.asfortranarray(rng.standard_normal((n, 3)))
    off = rng.uniform(-0.5, 0.5, n)
    v = None if wts == "unit" else rng.uniform(0.25, 4.0, n)
    if not presorted:
        dest = rng.permutation(n)
        for a in np.unique(first):
            b = a + sizes[gid[a]]
            dest[a:b] = np.sort(dest[a:b])
        inv = np.argsort(dest)                                   # row i holds sorted item inv[i]
        X, t, status, off, g = np.asfortranarray(X[inv]), t[inv], status[inv], off[inv], g[inv]
        v = None if v is None else v[inv]
    x = cd.SparseIterate(3)
    x[1], x[2], x[3] = 0.8, -0.6, 0.4
    for a in (X, t, status, off, g) + (() if v is None else (v,)):
        a.setflags(write=False)
    _DATA[key] = (X, t, status, off, g, v, x)
    return _DATA[key]


def _resend(f, t, status, off, g, v):
    """The same observations again, as _loss sent them: y and r back to zeros; the tie rule stays."""
    g32 = np.ascontiguousarray(g, dtype=np.int32) if np.any(g != g[0]) else None
    vn = None if v is None else np.ascontiguousarray(v * len(v) / v.sum())
    cd.check(f._L.cdh_glm_set_survival_strata(f._h, _vp(t), _vp(status), _vp(off), _vp(g32), _vp(vn)), f._h)
    f._synced = None


def _loss(monkeypatch, t, status, X, off, g, v, cap=FULL, ties="efron"):
    if cap != FULL:
        monkeypatch.setenv("CDH_COX_GRID", str(cap))            # read when the handle is made
    f = cd.CDCoxLoss(np.c_[t, status], X, off, strata=g if g is not None and np.any(g != g[0]) else None, weights=v)
    assert f.ties == "breslow"
    if ties is not None:
        f.set_ties(ties)
        assert f.ties == ties
    return f


def _bounds(n, q, eta_lin, tr):
    rho = q["rho"]
    bw = (10 * n + 84) * U * rho * q["eA"]
    bd = (4 * n + 66) * U * rho * (q["delta"] + q["eA"])
    br = (bd + np.abs(q["r"]) * bw) / np.where(tr, q["w"], 1.0)
    bz = br + U * np.abs(eta_lin)
    return bw, bd, br, bz


def _check_rows(tag, n, w, z, r, out, q, eta_lin, train, wmin, unit, ec):
    """w, z, r and the record against the twin's long-double rows q, by the bounds of the module's docstring.  Prints the worst
    multiples."""
    tr = np.ones(n, dtype=bool) if train is None else train
    bw, bd, br, bz = _bounds(n, q, eta_lin, tr)
    edge = tr & (np.abs(q["w_raw"] - wmin) <= bw)                # the clamp may go either way here
    sure = tr & ~edge
    unc = sure & ~q["clamped"]
    mw = (np.abs(w - q["w"])[unc] / bw[unc]).max() if unc.any() else 0.0
    nz = sure & (br > 0.0)
    mr = (np.abs(r - q["r"])[nz] / br[nz]).max() if nz.any() else 0.0
    mz = (np.abs(z - q["z"])[nz] / bz[nz]).max() if nz.any() else 0.0
    s_w = float(q["w"][tr].sum())
    m_sw = abs(out[1] - s_w) / ((n + 64) * U * s_w + float(bw[tr & (edge | ~q["clamped"])].sum()))
    s_dv = math.fsum(q["delta"])
    m_dv = abs(out[4] - s_dv) / ((n + 64) * U * s_dv) if s_dv > 0.0 else (0.0 if out[4] == 0.0 else np.inf)
    cnt = q["mm"] != 0.0
    mag = np.abs(q["mm"] * q["lg"]) + np.abs(q["delta"] * ec)
    b_nll = (2 * n + 66) * U * math.fsum(mag[cnt]) + math.fsum(q["mm"][cnt] * ((n + 11) * U * q["rho"][cnt] + 2 * U * np.abs(q["lg"][cnt])))
    err_nll = abs(out[0] - math.fsum(q["nll"][tr]))
    m_nll = err_nll / b_nll if b_nll > 0.0 else (0.0 if err_nll == 0.0 else np.inf)
    print(f"cox efron step {tag}: worst multiples of the bounds: w {mw:.3f} r {mr:.3f} z {mz:.3f} nll {m_nll:.3f} sum_w {m_sw:.3f} "
          f"sum_dv {m_dv:.3f}; largest rho {q['rho'].max():.3f}; clamped {int(out[2])} of {int(tr.sum())} (twin "
          f"{int(q['clamped'][tr].sum())}, {int(edge.sum())} within the bound of wmin) capped {int(out[3])} sum dv {out[4]:.6g}")
    assert mw <= 1.0 and mr <= 1.0 and mz <= 1.0 and m_nll <= 1.0 and m_sw <= 1.0 and m_dv <= 1.0
    np.testing.assert_array_equal(w[sure & q["clamped"]], wmin)
    np.testing.assert_array_equal(r[sure & (br == 0.0)], 0.0)
    assert abs(out[2] - q["clamped"][tr].sum()) <= edge.sum() and out[3] == q["capped"].sum()
    if unit:
        assert out[4] == q["delta"].sum()
    before = tr & (q["A"] == 0.0)
    np.testing.assert_array_equal(w[before], wmin)
    np.testing.assert_array_equal(r[before], 0.0)
    return unc


def _twin(eta_lin, off, t, status, g, vn, train=None, wmin=WMIN, emax=EMAX):
    return CE.rows(eta_lin, off, t, status, wmin, emax, train, strata=g, weights=vn, dtype=np.longdouble)


def _ec(eta_lin, off, emax=EMAX):
    return np.minimum(eta_lin + off, emax)


def _shape_is_what_the_pattern_says(n, cap, pattern, t, status, g):
    order, first, last, sfirst, slast = CS.groups(t, g)
    ev = status[order] != 0
    d = np.array([ev[first[s]:last[s] + 1].sum() for s in range(n)])
    if pattern == "none":
        assert np.all(first == last)
    elif pattern == "one":
        assert first.max() == 0 and last.min() == n - 1 and ev.all()
    elif n > 65:
        for b in _edges(n, cap):
            if not np.any(sfirst == b):                          # (a stratum that begins on the edge cannot be straddled)
                assert first[b] < b <= last[b] and last[b] - first[b] + 1 <= 7, (pattern, b)
        assert np.any((first // 4) != (last // 4))               # a lane's four positions
        assert d.max() >= 2
    if pattern == "strata" and n > 2:
        b = int(np.unique(sfirst)[1])
        assert b % 4 == 2 and t[order[b]] == t[order[b - 1]] and first[b] == b and last[b - 1] == b - 1
    if pattern == "noevent" and n > 2:
        assert not status[g == 4].any()
    if pattern in ("first", "last", "alternating") and n > 2:
        size = last - first + 1
        big = size >= 2
        pos = np.arange(n) - first
        want = {"first": pos < (size + 1) // 2, "last": pos >= size // 2, "alternating": pos % 2 == 0}[pattern]
        np.testing.assert_array_equal(ev[big], want[big])


# ---- the step, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,pattern", CASES, ids=IDS)
def test_step_row_by_row(monkeypatch, n, cap, pattern):
    for wts, presorted in COMBOS:
        X, t, status, off, g, v, x = _data(n, cap, pattern, wts, presorted)
        tag = "n%d-cap%d-%s-w%s-%s" % (n, cap, pattern, wts, "sorted" if presorted else "random")
        _shape_is_what_the_pattern_says(n, cap, pattern, t, status, g)
        f = _loss(monkeypatch, t, status, X, off, g, v, cap)
        vn = f.weights
        cd.initialize_(f, x)
        eta_lin = f.y - f.r
        q = _twin(eta_lin, off, t, status, g, vn)
        ro = _step(f, -1, 0, WMIN, EMAX)
        out = _step(f, -1, 1, WMIN, EMAX)
        assert np.array_equal(ro, out)                           # the read-only form takes the same sums, bit for bit
        w, z, r = f.w, f.y, f.r
        unc = _check_rows(tag, n, w, z, r, out, q, eta_lin, None, WMIN, v is None, _ec(eta_lin, off))
        if n >= 65 and pattern not in ("noevent",):
            assert unc.sum() >= n / 4, (int(unc.sum()), n)       # the w check is not vacuous
        if pattern == "noevent" and n > 2:
            m = g == 4
            assert np.all(q["A"][m] == 0.0)
            np.testing.assert_array_equal(w[m], WMIN)
            np.testing.assert_array_equal(r[m], 0.0)
        _step(f, -1, 0, WMIN, EMAX)                              # apply = 0 changes no bit of w, y, r
        for a, b in ((f.w, w), (f.y, z), (f.r, r)):
            np.testing.assert_array_equal(a, b)
        if pattern == "none":
            # without ties Efron is Breslow: the same handle's Breslow step within the bounds (not the bits: an event row adds
            # its own group's term last)
            f.set_ties("breslow")
            _resend(f, t, status, off, g, v)
            cd.initialize_(f, x)
            outb = _step(f, -1, 1, WMIN, EMAX)
            bw, bd, br, bz = _bounds(n, q, eta_lin, np.ones(n, dtype=bool))
            same = ~(np.abs(q["w_raw"] - WMIN) <= bw)
            assert np.all(np.abs(f.w - w)[same] <= 2 * bw[same]) and np.all(np.abs(f.r - r)[same] <= 2 * br[same])
            assert np.all(np.abs(f.y - z)[same] <= 2 * bz[same]) and outb[4] == out[4] and outb[3] == out[3]
            f.set_ties("efron")
        _pads_are_zero(f, n, w, z, r)
        f.close()


# ---- folds -------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [(n, cap, pat) for n, cap in ((65, FULL), (2 * T + 1, FULL)) for pat in PATTERNS]
FOLD_IDS = ["n%d-cap%d-%s" % c for c in FOLD_CASES]


def _fold_ids(n, t, status, g, k):
    """Random folds, then: one group with at least two events has ALL its events held out (it must add no hazard and no nll
    term), and one group with exactly two events has exactly one of them held out (it then behaves as d = 1).  -> (ids, the rows
    of the first group or None, the rows of the second or None)."""
    ids = np.random.default_rng(n).permutation(n) % 3
    order, first, last, _, _ = CS.groups(t, g)
    ev = status[order] != 0
    gone = half = None
    for a in np.unique(first):
        rows = order[a:last[a] + 1]
        events = rows[ev[a:last[a] + 1]]
        if gone is None and len(events) >= 2 and len(rows) > len(events):
            ids[events] = k
            ids[np.setdiff1d(rows, events)] = (k + 1) % 3
            gone = rows
        elif half is None and len(events) == 2:
            ids[events[0]], ids[events[1]] = k, (k + 1) % 3
            half = rows
    return ids, gone, half


@pytest.mark.parametrize("n,cap,pattern", FOLD_CASES, ids=FOLD_IDS)
def test_fold_groups_count_their_training_rows_only(monkeypatch, n, cap, pattern):
    """With fold k held out: held rows get w = 0, r = 0 and z = eta exactly; the training rows agree, within the bounds of the
    step, with the twin evaluated on the training rows ALONE -- so a group's d, D and m count training rows only."""
    k = 1
    for wts, presorted in COMBOS:
        X, t, status, off, g, v, x = _data(n, cap, pattern, wts, presorted)
        ids, gone, half = _fold_ids(n, t, status, g, k)
        if pattern in ("straddle", "alternating", "strata", "noevent"):
            assert gone is not None and half is not None, pattern
        train = ids != k
        if not status[train].any():
            continue
        f = _loss(monkeypatch, t, status, X, off, g, v, cap)
        f.set_folds(ids, 3)
        vn = f.weights
        cd.initialize_(f, x)
        eta_lin = f.y - f.r
        q = _twin(eta_lin, off, t, status, g, vn, train)
        alone = _twin(eta_lin[train], off[train], t[train], status[train], g[train], vn[train])
        for key in ("w", "r", "z", "nll"):
            np.testing.assert_array_equal(q[key][train], alone[key])  # (the twin's own statement of "the training rows alone")
        if gone is not None:                                     # the group whose events are all held out: no term anywhere
            assert not q["mm"][gone].any() and not q["nll"][gone].any()
        ro = _step(f, k, 0, WMIN, EMAX)
        out = _step(f, k, 1, WMIN, EMAX)
        assert np.array_equal(ro, out)
        w, z, r = f.w, f.y, f.r
        np.testing.assert_array_equal(w[~train], 0.0)
        np.testing.assert_array_equal(r[~train], 0.0)
        np.testing.assert_array_equal(z[~train], eta_lin[~train])
        tag = "fold n%d-%s-w%s-%s" % (n, pattern, wts, "sorted" if presorted else "random")
        _check_rows(tag, n, w, z, r, out, q, eta_lin, train, WMIN, v is None, _ec(eta_lin, off))
        _pads_are_zero(f, n, w, z, r)
        f.close()


# ---- the handle ----------------------------------------------------------------------------------------------------------------
def _bits(f, x, k=-1):
    """Both forms of the step at x.  The handle's y must be what a setter of survival data leaves (zeros): an applied step
    turns it into z, and eta_lin = y - r then rounds otherwise."""
    f._synced = None
    cd.initialize_(f, x)
    ro = _step(f, k, 0, WMIN, EMAX)
    out = _step(f, k, 1, WMIN, EMAX)
    return ro, out, f.w, f.y, f.r


def _same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("n,cap,wts,strata", ((65, FULL, "unit", False), (2 * T + 1, FULL, "random", True), (5 * T + 3, 2, "unit", False)))
def test_breslow_after_efron_is_the_breslow_step_bit_for_bit(monkeypatch, n, cap, wts, strata):
    """set_ties("breslow") after set_ties("efron") gives the Breslow step of a fresh handle, compared with == -- on a plain handle
    too, which Efron has turned into a segmented one over one stratum and unit weights.  Two Efron steps are bit-identical, on
    one handle and on two."""
    X, t, status, off, g, v, x = _data(n, cap, "strata" if strata else "straddle", wts, False)
    fresh = _loss(monkeypatch, t, status, X, off, g, v, cap, ties=None)
    want = _bits(fresh, x)
    fresh.close()
    f = _loss(monkeypatch, t, status, X, off, g, v, cap)
    e1 = _bits(f, x)
    _resend(f, t, status, off, g, v)
    assert f.ties == "efron"
    e2 = _bits(f, x)
    _same(e1, e2)
    f.set_ties("breslow")
    assert f.ties == "breslow"
    _resend(f, t, status, off, g, v)
    got = _bits(f, x)
    _same(want, got)
    assert not np.array_equal(got[2], e1[2])
    f.set_ties("efron")
    _resend(f, t, status, off, g, v)
    _same(e1, _bits(f, x))
    np.testing.assert_array_equal(f.strata, g if strata else np.zeros(n, dtype=np.int32))
    f.close()
    f2 = _loss(monkeypatch, t, status, X, off, g, v, cap)
    _same(e1, _bits(f2, x))
    f2.close()


def test_setters_keep_or_drop_the_rule_and_refusals_leave_the_handle_unchanged(monkeypatch):
    n = T + 1
    X, t, status, off, g, v, x = _data(n, FULL, "strata", "random", False)
    f = _loss(monkeypatch, t, status, X, off, g, v)
    L, h = f._L, f._h
    vn = f.weights
    g32 = np.ascontiguousarray(g, dtype=np.int32)
    efron = _bits(f, x)
    code = C.c_int32(-1)

    def rule():
        assert L.cdh_glm_get_cox_ties(h, C.byref(code)) == OK
        return code.value

    def refused(status_code, word=None):
        assert status_code == BAD and len(L.cdh_last_error(h)) > 0
        if word is not None:
            assert word.encode() in L.cdh_last_error(h), L.cdh_last_error(h)

    # refusals: an unknown rule, NULL pointers; the rule and the step's bits stay
    for bad in (2, -1, 7):
        refused(L.cdh_glm_set_cox_ties(h, bad), "ties must be 0 (Breslow) or 1 (Efron)")
    refused(L.cdh_glm_get_cox_ties(h, None))
    assert L.cdh_glm_set_cox_ties(None, 1) == BAD and L.cdh_glm_get_cox_ties(None, C.byref(code)) == BAD
    assert rule() == 1
    # cdh_glm_set_survival_strata keeps the rule (and so does cdh_glm_set_survival, which stores the defaults)
    cd.check(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    assert rule() == 1
    _same(efron, _bits(f, x))
    cd.check(L.cdh_glm_set_survival(h, _vp(t), _vp(status), _vp(off)), h)
    assert rule() == 1
    np.testing.assert_array_equal(f.strata, np.zeros(n, dtype=np.int32))
    np.testing.assert_array_equal(f.weights, np.ones(n))
    f._weighted = False
    plain = _loss(monkeypatch, t, status, X, off, None, None)
    _same(_bits(plain, x), _bits(f, x))
    plain.close()
    # start times put the handle back to Breslow, and Efron is then refused with a message that says why
    start = t - 0.25
    cd.check(L.cdh_glm_set_survival_interval(h, _vp(start), _vp(t), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    assert rule() == 0
    before = _step(f, -1, 0)
    refused(L.cdh_glm_set_cox_ties(h, 1), "start-stop times")
    assert rule() == 0 and np.array_equal(_step(f, -1, 0), before)
    # without start times the same setter keeps the rule
    cd.check(L.cdh_glm_set_survival_interval(h, None, _vp(t), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    assert rule() == 0
    cd.check(L.cdh_glm_set_cox_ties(h, 1), h)
    cd.check(L.cdh_glm_set_survival_interval(h, None, _vp(t), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    assert rule() == 1
    f._weighted = True
    _same(efron, _bits(f, x))
    # cdh_glm_set_labels drops it: not a Cox handle any more, and Breslow when survival data come back
    labels = (np.random.default_rng(0).random(n) < 0.5).astype(np.float64)
    cd.check(L.cdh_glm_set_labels(h, 0, _vp(labels)), h)
    refused(L.cdh_glm_get_cox_ties(h, C.byref(code)), "no survival data")
    refused(L.cdh_glm_set_cox_ties(h, 1), "no survival data")
    cd.check(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    assert rule() == 0
    fresh = _loss(monkeypatch, t, status, X, off, g, v, ties=None)
    _same(_bits(fresh, x), _bits(f, x))
    fresh.close()
    f.close()
