"""The Cox step with start-stop times on the device: cdh_glm_set_survival_interval, cdh_glm_get_survival_start and
cdh_glm_cox_irls over the interval chain (k_cox_exp<true> -> k_cox_gather -> the segmented offsets and suffix scans of T and T2
-> k_cox_hazard_iv -> the prefix scans -> k_cox_apply_iv), held row by row to the numpy twin's explicit risk sets
(tests/_cox_interval_numpy.scans_exact; its forms are pinned in tests/test_cox_interval_plan_host.py) at the eta the handle
held.

The bounds start from tests/test_gpu_cox_strata.py's docstring, with T + T2 in place of S and P(stop) + P(start) in place of A
and B wherever a difference is taken.  U = 2^-53, the twin's math.fsum values taken as exact, first order in U; the sizes
Ssz = T + T2, Asz = P_A(stop) + P_A(start), Bsz = P_B(stop) + P_B(start) are read off the twin's O(n) form (sums of positive
terms: within n U of themselves, a second-order term here).  All of it inside the row's own stratum.
    T, T2            each a segmented suffix scan of ev, the strata test's S:  |dT| <= (n + 10) U T, |dT2| <= (n + 10) U T2.
    S = T - T2       one more rounding, U |S| <= U (T + T2):                   |dS| <= (n + 11) U Ssz.
                     Relative to S itself that is (n + 11) U rho_k at event k, rho_k = Ssz_k / S_k;  rho = the largest rho_k
                     among the training events of the row's STRATUM (measured from the twin; the case's largest is printed: up
                     to ~20 with strata of many rows, hundreds where the "cycling" strata of 1..7 rows leave one small row at risk).
    P_A(u)           the strata test's A, |dA| <= (2n + 18) U A, is (n + 10) U for S's error in every term plus (n + 8) U for the
                     division and the prefix scan; with S's error (n + 11) U rho in place of the first:
                                                                              |dP_A| <= ((n + 11) rho + n + 8) U P_A.
    A = P(stop) - P(start)   both carry that, and the subtraction rounds once, U |A| <= U Asz:
                                                                              |dA| <= cA U Asz,  cA = (n + 11) rho + n + 9.
    B                the strata test's (3n + 20) U is twice (n + 10) U for S^2 plus n U; likewise
                                                                              |dB| <= cB U Bsz,  cB = (2n + 22) rho + n + 1.
    w (unclamped)    evA - ev (ev B).  The strata test's (5n + 76) U evA is its A bound, its B bound and 38 U for the products, ev
                     and the difference, relative to evA >= ev (ev B).  Here the A and B bounds are the ones above and the 38 U
                     stay relative to the two products:       |dw| <= bw = ev cA U Asz + ev^2 cB U Bsz + 38 U (evA + ev (ev B)).
    d = dv - evA     the strata test's (2n + 68) U (dv + evA) is its A bound plus 50 U:
                                                                              |dd| <= bd = ev cA U Asz + 50 U (dv + evA).
    r, z             as there:  |dr| <= (bd + |r| bw) / w,  |dz| <= that + U |eta_lin|.
    clamped          a row is clamped where w_raw < wmin; the device and the twin may disagree only where the twin's w_raw is
                     within bw of wmin ("near" rows).  Elsewhere a clamped row holds wmin itself and the counts agree.
    sum w            the record adds the DEVICE's w: (n + 64) U sum w for the addition, as there, plus the rows' own errors,
                     sum of bw over the unclamped and the near rows.
    sum dv           (n + 64) U sum dv -- and EXACT, compared with ==, where no weights were given.
    nll              the terms are dv (log S - ec).  log S carries S's relative error, (n + 11) U rho_k, and the library's log is
                     within an ulp, 2 U |log S|; the record's addition and the product are the strata test's (n + 65) U sum |terms|:
                     |dnll| <= (n + 65) U sum |terms| + sum over the events of dv ((n + 11) U rho_k + 2 U |log S_k|).
A row with Asz = 0 (no event of its stratum at or before its stop) has A = B = 0 exactly: w = wmin and r = 0, compared
with ==.  A row with Asz > 0 and A = 0 (no event inside its interval) has the difference of two prefix sums that differ by zero
terms only: they need not be the same bits on the device (the scan's tree groups them differently), so such a row is held to
the bounds, not to zero.
Every case prints rho and the worst measured multiple of its bounds; LAB_NOTES.md "Cox lasso: start-stop times" holds the ones
seen on an MI355X.  Every case with n >= 65 asserts that at least half of its training rows are unclamped in the twin (checked
on the CPU when the cases were chosen), so the w check is never vacuous."""
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_interval_numpy as CI
import _cox_plan as CP
from test_gpu_cox import _pads_are_zero, _step, _vp
from test_gpu_cox_strata import _sizes

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
T = CP.TILE
FULL = CP.MAX_GRID
WMIN, EMAX = 1e-5, 1.5                       # eta_max = 1.5: the rows above it cap ("scale" runs at 50: its point is e^30)

# (n, grid cap, strata pattern, ties, weights, presorted, probability of a start at 0)
CASES = [
    (1, FULL, "lane", "distinct", "none", False, 0.0), (1, FULL, "lane", "rounded", "uniform", True, 0.3),
    (2, FULL, "lane", "distinct", "uniform", False, 0.3), (2, FULL, "cycling", "rounded", "none", True, 0.0),
    (65, FULL, "lane", "distinct", "uniform", False, 0.3), (65, FULL, "cycling", "rounded", "none", True, 0.3),
    (65, FULL, "noevent", "rounded", "uniform", False, 0.0), (65, FULL, "scale", "distinct", "none", True, 0.3),
    (T + 1, FULL, "lane", "rounded", "uniform", True, 0.0), (T + 1, FULL, "tile", "distinct", "none", False, 0.3),
    (T + 1, FULL, "cycling", "rounded", "uniform", False, 0.3), (T + 1, FULL, "scale", "rounded", "uniform", True, 0.0),
    (2 * T + 1, FULL, "tile", "rounded", "uniform", False, 0.0), (2 * T + 1, FULL, "cycling", "distinct", "none", True, 0.3),
    (2 * T + 1, FULL, "noevent", "distinct", "uniform", True, 0.3), (2 * T + 1, FULL, "lane", "rounded", "none", False, 0.3),
    (5 * T + 3, 2, "tile", "distinct", "uniform", True, 0.3), (5 * T + 3, 2, "cycling", "rounded", "none", False, 0.0),
    (5 * T + 3, 2, "scale", "distinct", "uniform", False, 0.3), (5 * T + 3, 2, "lane", "rounded", "uniform", True, 0.3),
    (5 * T + 3, 2, "noevent", "rounded", "none", False, 0.0),
]
IDS = ["n%d-cap%d-%s-%s-w%s-%s-zero%g" % (n, cap, pat, ties, wts, "sorted" if s else "random", z)
       for n, cap, pat, ties, wts, s, z in CASES]

_DATA = {}


def _data(n, cap, pattern, ties, wts, presorted, zero):
    """X, start, stop, status, offset by the recipe of _cox_interval_numpy.make_data, strata ids by the strata test's patterns,
    weights (None, or uniform in [0.25, 4]) and the iterate beta = (0.8, -0.6, 0.4); computed once per case, left unchanged."""
    key = (n, cap, pattern, ties, wts, presorted, zero)
    if key in _DATA:
        return _DATA[key]
    X, start, stop, status, off = CI.make_data(n, 3, 3000 + n + 7 * len(pattern), rounded=ties == "rounded", zero=zero)
    status = status.copy()
    rng = np.random.default_rng(4000 + n + 7 * len(pattern))
    sizes = _sizes(n, cap, pattern)
    g = np.repeat(3 * np.arange(len(sizes)) - 4, sizes)[rng.permutation(n)]
    if pattern == "noevent":
        status[g == -1] = 0.0                                    # the middle stratum holds no event
    if pattern == "scale":
        off = off + 30.0 * (g == g.max())
    if not status.any():
        status[0] = 1.0
    v = None if wts == "none" else rng.uniform(0.25, 4.0, n)
    if presorted:
        o = np.lexsort((stop, g))
        X, start, stop, status, off, g = np.asfortranarray(X[o]), start[o], stop[o], status[o], off[o], g[o]
        v = None if v is None else v[o]
    x = cd.SparseIterate(3)
    x[1], x[2], x[3] = CI.BETA0
    for a in (X, start, stop, status, off, g) + (() if v is None else (v,)):
        a.setflags(write=False)
    _DATA[key] = (X, start, stop, status, off, g, v, x)
    return _DATA[key]


def _loss(monkeypatch, start, stop, status, X, off, g, v, cap=FULL):
    if cap != FULL:
        monkeypatch.setenv("CDH_COX_GRID", str(cap))            # read when the handle is made
    y = np.c_[stop, status] if start is None else np.c_[start, stop, status]
    return cd.CDCoxLoss(y, X, off, strata=g, weights=v)


def _emax(pattern):
    return 50.0 if pattern == "scale" else EMAX


def _check_rows(tag, n, g, w, z, r, out, q, sz, eta_lin, train, wmin, unit):
    """w, z, r and the record against the twin's exact rows q (sz: the twin's O(n) rows, for the sizes), by the bounds of the
    module's docstring.  Prints rho and the worst multiples."""
    tr = np.ones(n, dtype=bool) if train is None else train
    ev = q["delta"] != 0.0
    assert np.all(q["S"][ev] > 0.0)
    rho_k = sz["S_size"][ev] / q["S"][ev]
    _, sid = np.unique(g, return_inverse=True)
    rho_s = np.ones(sid.max() + 1)                               # per stratum (1 where it holds no event: nothing is divided there)
    np.maximum.at(rho_s, sid[ev], rho_k)
    rho = rho_s[sid]
    cA, cB = (n + 11) * rho + n + 9, (2 * n + 22) * rho + n + 1
    e = q["e"]                                                   # ev of the training rows (0 elsewhere: not checked there)
    bw = e * cA * U * sz["A_size"] + e * e * cB * U * sz["B_size"] + 38 * U * (q["eA"] + e * (e * q["B"]))
    bd = e * cA * U * sz["A_size"] + 50 * U * (q["delta"] + q["eA"])
    br = (bd + np.abs(q["r"]) * bw) / np.where(tr, q["w"], 1.0)
    bz = br + U * np.abs(eta_lin)
    near = tr & (np.abs(q["w_raw"] - wmin) <= bw)
    unc = tr & ~q["clamped"]
    free = tr & (~q["clamped"] | near)                           # rows whose w is not pinned to wmin on both sides
    mw = (np.abs(w - q["w"])[free] / bw[free]).max() if free.any() else 0.0
    nz = tr & (br > 0.0)
    mr = (np.abs(r - q["r"])[nz] / br[nz]).max() if nz.any() else 0.0
    mz = (np.abs(z - q["z"])[nz] / bz[nz]).max() if nz.any() else 0.0
    s_w = float(q["w"][tr].sum())
    m_sw = abs(out[1] - s_w) / ((n + 64) * U * s_w + float(bw[free].sum()))
    s_dv = math.fsum(q["delta"])
    m_dv = abs(out[4] - s_dv) / ((n + 64) * U * s_dv) if s_dv > 0.0 else (0.0 if out[4] == 0.0 else np.inf)
    err_nll = abs(out[0] - math.fsum(q["nll"][tr]))
    b_nll = (n + 65) * U * math.fsum(np.abs(q["nll"][tr])) + math.fsum(
        q["delta"][ev] * ((n + 11) * U * rho_k + 2 * U * np.abs(np.log(q["S"][ev]))))
    m_nll = err_nll / b_nll if b_nll > 0.0 else (0.0 if err_nll == 0.0 else np.inf)
    worst = max(mw, mr, mz, m_nll, m_sw, m_dv)
    print(f"cox interval step {tag}: rho {rho_s.max():.2f}; worst multiples of the bounds: w {mw:.4f} r {mr:.4f} z {mz:.4f} nll {m_nll:.4f} "
          f"sum_w {m_sw:.4f} sum_dv {m_dv:.4f} (worst {worst:.4f}); clamped {int(out[2])} of {int(tr.sum())} near {int(near.sum())} "
          f"capped {int(out[3])} sum dv {out[4]:.6g}")
    assert mw <= 1.0 and mr <= 1.0 and mz <= 1.0 and m_nll <= 1.0 and m_sw <= 1.0 and m_dv <= 1.0
    # exact facts
    pinned = tr & q["clamped"] & ~near
    np.testing.assert_array_equal(w[pinned], wmin)
    assert abs(out[2] - q["clamped"][tr].sum()) <= near.sum() and out[3] == q["capped"].sum()
    if unit:
        assert out[4] == q["delta"].sum()
    before = tr & (sz["A_size"] == 0.0)
    np.testing.assert_array_equal(w[before], wmin)
    np.testing.assert_array_equal(r[before], 0.0)
    if n >= 65:
        assert unc.sum() >= tr.sum() / 2, (int(unc.sum()), int(tr.sum()))
    return worst


def _twin(eta_lin, off, start, stop, status, emax, train, g, vn):
    q = CI.rows(eta_lin, off, start, stop, status, WMIN, emax, train, exact=True, strata=g, weights=vn)
    sz = CI.rows(eta_lin, off, start, stop, status, WMIN, emax, train, strata=g, weights=vn)
    return q, sz


# ---- the step, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,pattern,ties,wts,presorted,zero", CASES, ids=IDS)
def test_step_row_by_row(monkeypatch, n, cap, pattern, ties, wts, presorted, zero):
    X, start, stop, status, off, g, v, x = _data(n, cap, pattern, ties, wts, presorted, zero)
    tag = IDS[CASES.index((n, cap, pattern, ties, wts, presorted, zero))]
    emax = _emax(pattern)
    if ties == "rounded" and n >= 65:                            # starts coincide with event times, and with each other
        assert np.isin(start, stop[status == 1.0]).any() and len(np.unique(start)) < n
    f = _loss(monkeypatch, start, stop, status, X, off, g, v, cap)
    np.testing.assert_array_equal(f.start, start)               # the getters round-trip, in the caller's row order
    np.testing.assert_array_equal(f.time, stop)
    np.testing.assert_array_equal(f.status, status)
    np.testing.assert_array_equal(f.offset, off)
    np.testing.assert_array_equal(f.strata, g)
    vn = f.weights
    np.testing.assert_array_equal(vn, np.ones(n) if v is None else v * n / v.sum())
    cd.initialize_(f, x)
    eta_lin = f.y - f.r                                          # what the kernels recover, from the same two stored vectors
    q, sz = _twin(eta_lin, off, start, stop, status, emax, None, g, vn)
    ro = _step(f, -1, 0, WMIN, emax)
    ro2 = _step(f, -1, 0, WMIN, emax)
    out = _step(f, -1, 1, WMIN, emax)
    assert np.array_equal(ro, ro2) and np.array_equal(ro, out)  # two read-only steps and the applied one: the same sums, bit for bit
    w, z, r = f.w, f.y, f.r
    _check_rows(tag, n, g, w, z, r, out, q, sz, eta_lin, None, WMIN, unit=v is None)
    if pattern == "noevent":
        m = g == -1
        assert np.all(sz["A_size"][m] == 0.0)
        np.testing.assert_array_equal(w[m], WMIN)
        np.testing.assert_array_equal(r[m], 0.0)
    # apply = 0 changes no bit of w, y, r; the data are where they were
    _step(f, -1, 0, WMIN, emax)
    for a, b in ((f.w, w), (f.y, z), (f.r, r)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(f.start, start)
    np.testing.assert_array_equal(f.time, stop)
    _pads_are_zero(f, n, w, z, r)
    f.close()


# ---- folds -------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [c for c in CASES if (c[0], c[2]) in ((65, "cycling"), (65, "lane"), (T + 1, "tile"), (2 * T + 1, "cycling"),
                                                   (2 * T + 1, "noevent"), (5 * T + 3, "tile"), (5 * T + 3, "lane"))]
FOLD_IDS = [IDS[CASES.index(c)] for c in FOLD_CASES]
assert len(FOLD_CASES) == 7


@pytest.mark.parametrize("n,cap,pattern,ties,wts,presorted,zero", FOLD_CASES, ids=FOLD_IDS)
def test_fold_rows_leave_the_risk_sets(monkeypatch, n, cap, pattern, ties, wts, presorted, zero):
    """With fold 1 of 3 held out: held rows get w = 0, r = 0 and z = eta exactly and leave both sums of S and the hazards; the
    training rows agree, within the bounds of the step, with the twin evaluated on the training rows ALONE."""
    X, start, stop, status, off, g, v, x = _data(n, cap, pattern, ties, wts, presorted, zero)
    ids = np.random.default_rng(n).permutation(n) % 3
    k = 1
    train = ids != k
    assert status[train].any()
    f = _loss(monkeypatch, start, stop, status, X, off, g, v, cap)
    f.set_folds(ids, 3)
    vn = f.weights
    cd.initialize_(f, x)
    eta_lin = f.y - f.r
    q, sz = _twin(eta_lin, off, start, stop, status, EMAX, train, g, vn)
    alone = CI.rows(eta_lin[train], off[train], start[train], stop[train], status[train], WMIN, EMAX, None, exact=True,
                    strata=g[train], weights=vn[train])
    for key in ("w", "r", "z"):
        np.testing.assert_array_equal(q[key][train], alone[key])  # (the twin's own statement of "the training rows alone")
    ro = _step(f, k, 0, WMIN, EMAX)
    out = _step(f, k, 1, WMIN, EMAX)
    assert np.array_equal(ro, out)
    w, z, r = f.w, f.y, f.r
    np.testing.assert_array_equal(w[~train], 0.0)
    np.testing.assert_array_equal(r[~train], 0.0)
    np.testing.assert_array_equal(z[~train], eta_lin[~train])
    _check_rows("fold " + FOLD_IDS[FOLD_CASES.index((n, cap, pattern, ties, wts, presorted, zero))], n, g, w, z, r, out, q, sz, eta_lin,
                train, WMIN, unit=v is None)
    _pads_are_zero(f, n, w, z, r)
    f.close()


# ---- bit identity ------------------------------------------------------------------------------------------------------------
def _bits(f, x, k=-1, emax=EMAX):
    cd.initialize_(f, x)
    ro = _step(f, k, 0, WMIN, emax)
    out = _step(f, k, 1, WMIN, emax)
    return ro, out, f.w, f.y, f.r


def _same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("n,cap", ((65, FULL), (2 * T + 1, FULL), (5 * T + 3, 2)))
def test_starts_below_every_stop_are_the_strata_step_bit_for_bit(monkeypatch, n, cap):
    """w, z, r and out5 compared with ==: an interval handle whose starts all lie below every stop (lo = enter = -1: nothing
    is ever subtracted) against the strata handle on the same data, with strata and weights, and with neither (the interval
    handle then stores the defaults) against explicit single-stratum ids and unit weights; one fold held out too."""
    pattern = "cycling" if n != 2 * T + 1 else "tile"
    X, _, stop, status, off, g, v, x = _data(n, cap, pattern, "rounded", "uniform", False, 0.3)
    start = stop.min() - 1.0 - np.random.default_rng(n).random(n)
    ids = np.arange(n) % 3
    for gg, vv in ((g, v), (None, None)):
        ref = _loss(monkeypatch, None, stop, status, X, off, gg if gg is not None else np.zeros(n, dtype=np.int32),
                    vv if vv is not None else np.ones(n), cap)
        f = _loss(monkeypatch, start, stop, status, X, off, gg, vv, cap)
        np.testing.assert_array_equal(f.start, start)
        assert ref.start is None
        _same(_bits(ref, x), _bits(f, x))
        ref.set_folds(ids, 3)
        f.set_folds(ids, 3)
        ref._synced = f._synced = None
        _same(_bits(ref, x, 1), _bits(f, x, 1))
        ref.close()
        f.close()


def test_the_setter_with_a_null_start_is_the_strata_setter(monkeypatch):
    """On one handle: cdh_glm_set_survival_strata, then cdh_glm_set_survival_interval with start NULL -- the same bits, and no
    start times held; with every optional pointer NULL it is cdh_glm_set_survival."""
    n = 2 * T + 1
    X, start, stop, status, off, g, v, x = _data(n, FULL, "tile", "rounded", "uniform", False, 0.0)
    f = _loss(monkeypatch, None, stop, status, X, off, g, v)
    vn = f.weights
    g32 = np.ascontiguousarray(g, dtype=np.int32)
    want = _bits(f, x)
    L, h = f._L, f._h
    cd.check(L.cdh_glm_set_survival_interval(h, None, _vp(stop), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    f._synced = None
    _same(want, _bits(f, x))
    assert L.cdh_glm_get_survival_start(h, _vp(np.zeros(n))) == BAD
    np.testing.assert_array_equal(f.strata, g)
    plain = cd.CDCoxLoss(np.c_[stop, status], X, off)
    want = _bits(plain, x)
    cd.check(L.cdh_glm_set_survival_interval(h, None, _vp(stop), _vp(status), _vp(off), None, None), h)
    f._synced = None
    f._weighted = False
    _same(want, _bits(f, x))
    np.testing.assert_array_equal(f.strata, np.zeros(n, dtype=np.int32))
    plain.close()
    f.close()


def test_repeatable_across_handles(monkeypatch):
    """Two identical steps on two handles, each read-only twice and applied: the same bits."""
    n, cap = 5 * T + 3, 2
    X, start, stop, status, off, g, v, x = _data(n, cap, "cycling", "rounded", "none", False, 0.0)
    got = []
    for _ in range(2):
        f = _loss(monkeypatch, start, stop, status, X, off, g, v, cap)
        cd.initialize_(f, x)
        a, b = _step(f, -1, 0), _step(f, -1, 0)
        assert np.array_equal(a, b)
        got.append(_bits(f, x))
        assert np.array_equal(a, got[-1][0])
        f.close()
    _same(got[0], got[1])


# ---- the handle's other lives, and the refusals ----------------------------------------------------------------------------------
def test_the_older_setters_drop_the_start_times(monkeypatch):
    """cdh_glm_set_survival, cdh_glm_set_survival_strata, cdh_glm_set_labels and cdh_glm_set_counts after the new setter: the
    start getter is refused, and the step is a fresh handle's without starts, bit for bit; the new setter brings the starts back
    on the same buffers."""
    n = T + 1
    X, start, stop, status, off, g, v, x = _data(n, FULL, "tile", "distinct", "none", False, 0.3)
    v = np.random.default_rng(5).uniform(0.25, 4.0, n)
    f = _loss(monkeypatch, start, stop, status, X, off, g, v)
    with_start = _bits(f, x)
    vn = f.weights
    g32 = np.ascontiguousarray(g, dtype=np.int32)
    L, h = f._L, f._h
    buf = np.zeros(n)

    def again():
        cd.check(L.cdh_glm_set_survival_interval(h, _vp(start), _vp(stop), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
        assert L.cdh_glm_get_survival_start(h, _vp(buf)) == OK
        np.testing.assert_array_equal(buf, start)

    # cdh_glm_set_survival
    cd.check(L.cdh_glm_set_survival(h, _vp(stop), _vp(status), _vp(off)), h)
    assert L.cdh_glm_get_survival_start(h, _vp(buf)) == BAD and b"start" in L.cdh_last_error(h)
    f._synced, f._weighted = None, False
    fresh = cd.CDCoxLoss(np.c_[stop, status], X, off)
    _same(_bits(fresh, x), _bits(f, x))
    fresh.close()
    again()
    # cdh_glm_set_survival_strata
    cd.check(L.cdh_glm_set_survival_strata(h, _vp(stop), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    assert L.cdh_glm_get_survival_start(h, _vp(buf)) == BAD
    f._synced, f._weighted = None, True
    fresh = cd.CDCoxLoss(np.c_[stop, status], X, off, strata=g, weights=v)
    got = _bits(f, x)
    _same(_bits(fresh, x), got)
    assert not np.array_equal(got[2], with_start[2])
    fresh.close()
    again()
    # cdh_glm_set_labels and cdh_glm_set_counts: not a Cox handle any more; back through the plain setter: still no starts
    labels = (np.random.default_rng(0).random(n) < 0.5).astype(np.float64)
    for setter in (lambda: L.cdh_glm_set_labels(h, 0, _vp(labels)), lambda: L.cdh_glm_set_counts(h, _vp(labels), None)):
        cd.check(setter(), h)
        assert L.cdh_glm_get_survival_start(h, _vp(buf)) == BAD
        cd.check(L.cdh_glm_set_survival_strata(h, _vp(stop), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
        assert L.cdh_glm_get_survival_start(h, _vp(buf)) == BAD
        again()
    assert L.cdh_glm_get_survival_start(h, None) == BAD and L.cdh_glm_get_survival_start(None, _vp(buf)) == BAD
    f._synced = None
    _same(with_start, _bits(f, x))
    f.close()


def test_refusals_leave_the_handle_unchanged(monkeypatch):
    n = 65
    X, start, stop, status, off, g, v, x = _data(n, FULL, "lane", "distinct", "uniform", False, 0.3)
    f = _loss(monkeypatch, start, stop, status, X, off, g, v)
    cd.initialize_(f, x)
    _step(f, -1, 1)
    before = _step(f, -1, 0)
    y0, w0, r0 = f.y, f.w, f.r
    vn = f.weights
    L, h = f._L, f._h
    g32 = np.ascontiguousarray(g, dtype=np.int32)

    def refused(status_code, word=None):
        assert status_code == BAD
        assert len(L.cdh_last_error(h)) > 0
        if word is not None:
            assert word.encode() in L.cdh_last_error(h), L.cdh_last_error(h)

    def call(a=start, b=stop, c=status, o=off, gg=g32, vv=vn):
        return L.cdh_glm_set_survival_interval(h, _vp(a), _vp(b), _vp(c), _vp(o), _vp(gg), _vp(vv))

    for i, value in ((7, np.nan), (0, np.inf), (64, -np.inf)):
        bad = start.copy()
        bad[i] = value
        refused(call(a=bad), "start[%d]" % i)
    for i, value in ((3, stop[3]), (64, stop[64] + 1.0)):
        bad = start.copy()
        bad[i] = value
        refused(call(a=bad), "start[%d] = " % i)
        assert b"is not below stop[%d]" % i in L.cdh_last_error(h)
    # what cdh_glm_set_survival_strata refuses, with and without start times
    for a in (start, None):
        bad = stop.copy()
        bad[7] = np.nan
        refused(call(a=a, b=bad), "time[7]")
        bad = status.copy()
        bad[9] = 0.5
        refused(call(a=a, c=bad), "status[9]")
        bad = off.copy()
        bad[3] = np.inf
        refused(call(a=a, o=bad), "offset[3]")
        bad = vn.copy()
        bad[11] = 0.0
        refused(call(a=a, vv=bad), "weights[11]")
        refused(call(a=a, c=np.zeros(n)), "no row is an event")
        refused(call(a=a, b=None))
        refused(call(a=a, c=None))
    refused(L.cdh_glm_get_survival_start(h, None))
    assert L.cdh_glm_set_survival_interval(None, _vp(start), _vp(stop), _vp(status), None, None, None) == BAD
    np.testing.assert_array_equal(f.start, start)
    np.testing.assert_array_equal(f.time, stop)
    np.testing.assert_array_equal(f.status, status)
    np.testing.assert_array_equal(f.offset, off)
    np.testing.assert_array_equal(f.strata, g)
    np.testing.assert_array_equal(f.weights, vn)
    for a, b in ((f.y, y0), (f.w, w0), (f.r, r0)):              # y, w and r as the applied step left them
        np.testing.assert_array_equal(a, b)
    assert np.array_equal(_step(f, -1, 0), before)               # and the step's bits before and after the refused calls
    f.close()
