"""The Cox step with strata and observation weights on the device: cdh_glm_set_survival_strata, cdh_glm_get_survival_strata and
cdh_glm_cox_irls over the segmented instantiations of k_cox_exp, k_cox_offsets, k_cox_scan, k_cox_hazard and the weighted
k_cox_apply, held row by row to the numpy twin (tests/_cox_strata_numpy.py; its forms are pinned in
tests/test_cox_strata_plan_host.py) at the eta the handle held.

The bounds are those of tests/test_gpu_cox.py's docstring, RELATIVE TO THE STRATUM'S OWN S, A, B and evA -- which only a
scan that restarts at the stratum's boundary meets: a global scan with a subtraction at the boundary carries n U times the
LATER strata's sums into this stratum's S (the "scale" cases: the later stratum's e is e^30 times the earlier one's) --
widened by the roundings the weights add.  With U = 2^-53 and the twin's math.fsum values taken as exact:
    dv = v delta      is exact: delta is 0 or 1.
    ev = v e          one more rounding per scanned term: the device's ev is within 2 U of the twin's beyond what its e is
                      (its own rounding and the twin's), so  |dS| <= (n + 10) U S.
    A, B              their terms dv / S and dv / S^2 carry S's error once and twice: |dA| <= (2n + 18) U A,
                      |dB| <= (3n + 20) U B                                                           (not observable here)
    w (unclamped)     evA - ev (ev B): ev enters once beside A (2 U for ev, 2 U for A's S) and twice beside B (4 U, and 4 U for
                      B's S^2), 12 U in all relative to evA >= ev (ev B):  |dw| <= (5n + 76) U evA
    d = dv - evA      2 U for ev, 2 U for A:  |dd| <= (2n + 68) U (dv + evA)
    r, z              as there:  |dr| <= (|dd| bound + |r| |dw| bound) / w,  |dz| <= |dr| bound + U |eta_lin|
    sum w             (n + 64) U sum w, as there
    sum dv            (n + 64) U sum dv -- and EXACT, compared with ==, where every weight is 1 or none was given
    nll               the terms are dv (log S - ec): one more rounding each, U |term|, so (n + 65) U sum |terms|; held to that
                      bound wherever it is at least NLL_FLOOR and to NLL_FLOOR above it elsewhere (the rule of
                      tests/test_gpu_cox.py), NLL_FLOOR = sum over the events of dv ((n + 10) U + 2 U |log S|).
Every case prints the worst measured multiple of its bounds; LAB_NOTES.md "Cox lasso: strata and weights" holds the ones seen
on an MI355X.  Every case with n >= 65 asserts that at least half of its training rows are unclamped in the twin (the seeds
were chosen on the CPU for that), so the w check is never vacuous."""
import ctypes as C
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_plan as CP
import _cox_strata_numpy as CS
from test_gpu_cox import _pads_are_zero, _step, _vp      # (the plain step's call and its moment trick for the pad rows)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
T = CP.TILE
WMIN, EMAX = 1e-5, 1.5                       # eta_max = 1.5: the rows above it cap ("scale" runs at 50: its point is e^30)

# (n, grid cap, strata pattern, ties, weights, presorted)
FULL = CP.MAX_GRID
CASES = [
    (1, FULL, "lane", "distinct", "none", False), (1, FULL, "lane", "distinct", "uniform", False),
    (2, FULL, "lane", "distinct", "ones", False), (2, FULL, "cycling", "rounded", "uniform", True),
    (65, FULL, "lane", "distinct", "uniform", False), (65, FULL, "cycling", "rounded", "none", True),
    (65, FULL, "noevent", "rounded", "uniform", False), (65, FULL, "scale", "distinct", "ones", False),
    (T + 1, FULL, "lane", "rounded", "uniform", True), (T + 1, FULL, "wave", "distinct", "uniform", False),
    (T + 1, FULL, "tile", "rounded", "none", False), (T + 1, FULL, "cycling", "distinct", "uniform", False),
    (T + 1, FULL, "scale", "rounded", "uniform", True),
    (2 * T + 1, FULL, "wave", "rounded", "ones", True), (2 * T + 1, FULL, "tile", "distinct", "uniform", False),
    (2 * T + 1, FULL, "cycling", "rounded", "uniform", False), (2 * T + 1, FULL, "noevent", "distinct", "none", True),
    (5 * T + 3, 2, "run", "rounded", "uniform", False), (5 * T + 3, 2, "tile", "distinct", "none", True),
    (5 * T + 3, 2, "cycling", "rounded", "uniform", True), (5 * T + 3, 2, "scale", "distinct", "uniform", False),
    (5 * T + 3, 2, "lane", "rounded", "ones", False),
]
IDS = ["n%d-cap%d-%s-%s-w%s-%s" % (n, cap, pat, ties, wts, "sorted" if s else "random") for n, cap, pat, ties, wts, s in CASES]


def _sizes(n, cap, pattern):
    """The strata's sizes in sorted order."""
    if pattern == "cycling":                                     # several heads per lane and per wave
        out, k = [], 0
        while sum(out) < n:
            out.append(min(k % 7 + 1, n - sum(out)))
            k += 1
        return out
    if n <= 2:
        return [1] * n
    if pattern == "lane":                                        # a boundary inside a lane's four positions: size = 2 mod 4
        first = 2 if n <= 65 else 4 * (n // 8) + 2
    elif pattern == "wave":                                      # exactly on a wave's edge
        first = 256
    elif pattern == "tile":                                      # exactly on a tile's edge
        first = T
    elif pattern == "run":                                       # exactly on the edge between the capped grid's two runs
        pl = CP.plan(CP.padded(n), cap)
        first = CP.run_first(pl["tiles"], pl["grid"], 1) * T
    elif pattern == "noevent":
        return [n // 3, n // 3, n - 2 * (n // 3)]
    else:                                                        # "scale": two strata, the later one e^30 times the earlier
        first = n // 2
    assert 0 < first < n
    return [first, n - first]


_DATA = {}


def _data(n, cap, pattern, ties, wts, presorted):
    """X, time, status, offset, strata ids, weights (None, ones, or uniform in [0.25, 4]) and the iterate; computed once per
    case and left unchanged.  The ids are spread (negative, not consecutive), in ascending order of the strata's positions."""
    key = (n, cap, pattern, ties, wts, presorted)
    if key in _DATA:
        return _DATA[key]
    rng = np.random.default_rng(2000 + n + 7 * len(pattern))
    X = np.asfortranarray(rng.standard_normal((n, 3)))
    t = rng.exponential(1.0, n)
    if ties == "rounded":
        t = np.round(t, 1)
    status = (rng.random(n) < 0.7).astype(np.float64)
    off = rng.uniform(-0.5, 0.5, n)
    sizes = _sizes(n, cap, pattern)
    g = np.repeat(3 * np.arange(len(sizes)) - 4, sizes)[rng.permutation(n)]
    if pattern == "noevent":
        status[g == -1] = 0.0                                    # the middle stratum holds no event
    if pattern == "scale":
        off = off + 30.0 * (g == g.max())
    if not status.any():
        status[0] = 1.0
    v = None if wts == "none" else (np.ones(n) if wts == "ones" else rng.uniform(0.25, 4.0, n))
    if presorted:
        o = np.lexsort((t, g))
        X, t, status, off, g = np.asfortranarray(X[o]), t[o], status[o], off[o], g[o]
        v = None if v is None else v[o]
    x = cd.SparseIterate(3)
    x[1], x[2], x[3] = 0.8, -0.6, 0.4
    for a in (X, t, status, off, g) + (() if v is None else (v,)):
        a.setflags(write=False)
    _DATA[key] = (X, t, status, off, g, v, x)
    return _DATA[key]


def _loss(monkeypatch, t, status, X, off, g, v, cap=FULL):
    if cap != FULL:
        monkeypatch.setenv("CDH_COX_GRID", str(cap))            # read when the handle is made
    return cd.CDCoxLoss(np.c_[t, status], X, off, strata=g, weights=v)


def _emax(pattern):
    return 50.0 if pattern == "scale" else EMAX


def _check_rows(tag, n, w, z, r, out, q, eta_lin, train, wmin, unit):
    """w, z, r and the record against the twin's exact rows q, by the bounds of the module's docstring.  Prints the worst
    multiples."""
    tr = np.ones(n, dtype=bool) if train is None else train
    unc = tr & ~q["clamped"]
    bw = (5 * n + 76) * U * q["eA"]
    bd = (2 * n + 68) * U * (q["delta"] + q["eA"])
    br = (bd + np.abs(q["r"]) * bw) / np.where(tr, q["w"], 1.0)
    bz = br + U * np.abs(eta_lin)
    mw = (np.abs(w - q["w"])[unc] / bw[unc]).max() if unc.any() else 0.0
    nz = tr & (br > 0.0)
    mr = (np.abs(r - q["r"])[nz] / br[nz]).max() if nz.any() else 0.0
    mz = (np.abs(z - q["z"])[nz] / bz[nz]).max() if nz.any() else 0.0
    ev = q["delta"] != 0.0
    s_w = float(q["w"][tr].sum())
    m_sw = abs(out[1] - s_w) / ((n + 64) * U * s_w)
    s_dv = math.fsum(q["delta"])
    m_dv = abs(out[4] - s_dv) / ((n + 64) * U * s_dv) if s_dv > 0.0 else (0.0 if out[4] == 0.0 else np.inf)
    err_nll = abs(out[0] - math.fsum(q["nll"][tr]))
    plain = (n + 65) * U * math.fsum(np.abs(q["nll"][tr]))
    floor = math.fsum(q["delta"][ev] * ((n + 10) * U + 2 * U * np.abs(np.log(q["S"][ev]))))
    degenerate = plain < floor
    m_plain = err_nll / plain if plain > 0.0 else (0.0 if err_nll == 0.0 else np.inf)
    m_nll = err_nll / (plain + floor) if degenerate else m_plain
    print(f"cox strata step {tag}: worst multiples of the bounds: w {mw:.3f} r {mr:.3f} z {mz:.3f} nll {m_nll:.3f} sum_w {m_sw:.3f} "
          f"sum_dv {m_dv:.3f}; nll against (n + 65) U sum|terms| alone: {m_plain:.3f}"
          f"{' (DEGENERATE: below the floor, held to bound + floor)' if degenerate else ''}; clamped {int(out[2])} of "
          f"{int(tr.sum())} capped {int(out[3])} sum dv {out[4]:.6g}")
    assert mw <= 1.0 and mr <= 1.0 and mz <= 1.0 and m_nll <= 1.0 and m_sw <= 1.0 and m_dv <= 1.0
    # exact facts: the clamped rows hold wmin itself; rows where the bound is zero (A = 0: before their stratum's first event,
    # or in a stratum without one) hold r = 0; without weights, or with unit ones, the last slot is the event count
    np.testing.assert_array_equal(w[tr & q["clamped"]], wmin)
    np.testing.assert_array_equal(r[tr & (br == 0.0)], 0.0)
    assert out[2] == q["clamped"][tr].sum() and out[3] == q["capped"].sum()
    if unit:
        assert out[4] == q["delta"].sum()
    before = tr & (q["A"] == 0.0)
    np.testing.assert_array_equal(w[before], wmin)
    np.testing.assert_array_equal(r[before], 0.0)
    if n >= 65:
        assert unc.sum() >= tr.sum() / 2, (int(unc.sum()), int(tr.sum()))


def _boundaries(g, t):
    """Where the strata's boundaries lie, in sorted positions: -> the set of first positions of the strata after the first."""
    _, _, _, sfirst, _ = CS.groups(t, g)
    return set(int(a) for a in np.unique(sfirst) if a > 0)


# ---- the step, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,pattern,ties,wts,presorted", CASES, ids=IDS)
def test_step_row_by_row(monkeypatch, n, cap, pattern, ties, wts, presorted):
    X, t, status, off, g, v, x = _data(n, cap, pattern, ties, wts, presorted)
    tag = IDS[CASES.index((n, cap, pattern, ties, wts, presorted))]
    emax = _emax(pattern)
    edges = _boundaries(g, t)
    if n > 2:                                                    # the boundary is where the pattern says
        if pattern == "lane":
            assert len(edges) == 1 and min(edges) % 4 == 2
        elif pattern == "wave":
            assert edges == {256}
        elif pattern == "tile":
            assert edges == {T}
        elif pattern == "run":
            pl = CP.plan(CP.padded(n), cap)
            assert pl["grid"] == 2 and edges == {CP.run_first(pl["tiles"], 2, 1) * T} and min(edges) % T == 0
        elif pattern == "cycling":
            assert len(edges) >= n // 7 and any(a % 4 for a in edges)
    f = _loss(monkeypatch, t, status, X, off, g, v, cap)
    np.testing.assert_array_equal(f.time, t)
    np.testing.assert_array_equal(f.status, status)
    np.testing.assert_array_equal(f.offset, off)
    np.testing.assert_array_equal(f.strata, g)                  # the getter round-trips, in the caller's row order
    vn = f.weights
    if v is None or wts == "ones":
        np.testing.assert_array_equal(vn, np.ones(n))
    else:
        np.testing.assert_array_equal(vn, v * n / v.sum())      # normalised on the host, stored as given
    cd.initialize_(f, x)
    eta_lin = f.y - f.r                                          # what the kernels recover, from the same two stored vectors
    q = CS.rows(eta_lin, off, t, status, WMIN, emax, None, exact=True, strata=g, weights=vn)
    if pattern == "scale" and n > 2:                             # the later stratum's sums dwarf the earlier one's
        lo, hi = q["S"][g == g.min()].max(), q["S"][g == g.max()].max()
        assert hi > 1e12 * lo, (lo, hi)
    ro = _step(f, -1, 0, WMIN, emax)
    out = _step(f, -1, 1, WMIN, emax)
    assert np.array_equal(ro, out)                               # the read-only form takes the same sums, bit for bit
    w, z, r = f.w, f.y, f.r
    _check_rows(tag, n, w, z, r, out, q, eta_lin, None, WMIN, unit=v is None or wts == "ones")
    if pattern == "noevent":
        m = g == -1
        assert np.all(q["A"][m] == 0.0)
        np.testing.assert_array_equal(w[m], WMIN)
        np.testing.assert_array_equal(r[m], 0.0)
    # apply = 0 changes no bit of w, y, r; the data are where they were
    _step(f, -1, 0, WMIN, emax)
    for a, b in ((f.w, w), (f.y, z), (f.r, r)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(f.time, t)
    np.testing.assert_array_equal(f.strata, g)
    np.testing.assert_array_equal(f.weights, vn)
    _pads_are_zero(f, n, w, z, r)
    f.close()


# ---- folds -------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [c for c in CASES if (c[0], c[2]) in ((65, "cycling"), (65, "noevent"), (T + 1, "lane"), (T + 1, "tile"),
                                                   (2 * T + 1, "cycling"), (5 * T + 3, "run"), (5 * T + 3, "cycling"))]
FOLD_IDS = [IDS[CASES.index(c)] for c in FOLD_CASES]
assert len(FOLD_CASES) == 7


@pytest.mark.parametrize("n,cap,pattern,ties,wts,presorted", FOLD_CASES, ids=FOLD_IDS)
def test_fold_rows_leave_the_risk_sets_of_their_stratum(monkeypatch, n, cap, pattern, ties, wts, presorted):
    """With fold k held out: held rows get w = 0, r = 0 and z = eta exactly; the training rows agree, within the bounds of the
    step, with the twin evaluated on the training rows ALONE.  One whole stratum is held out too (the second one; with
    "cycling" every stratum whose id is 2 mod 4 in the count): its rows hold zeros and nobody else's sums see it."""
    X, t, status, off, g, v, x = _data(n, cap, pattern, ties, wts, presorted)
    ids = np.random.default_rng(n).permutation(n) % 3
    k = 1
    gone = (g == np.unique(g)[1]) if pattern != "cycling" else (((g + 4) // 3) % 4 == 2)
    ids = np.where(gone, k, ids)
    train = ids != k
    assert gone.any() and not train[gone].any() and status[train].any()
    f = _loss(monkeypatch, t, status, X, off, g, v, cap)
    f.set_folds(ids, 3)
    vn = f.weights
    cd.initialize_(f, x)
    eta_lin = f.y - f.r
    q = CS.rows(eta_lin, off, t, status, WMIN, EMAX, train, exact=True, strata=g, weights=vn)
    alone = CS.rows(eta_lin[train], off[train], t[train], status[train], WMIN, EMAX, None, exact=True, strata=g[train],
                    weights=vn[train])
    for key in ("w", "r", "z"):
        np.testing.assert_array_equal(q[key][train], alone[key])  # (the twin's own statement of "the training rows alone")
    ro = _step(f, k, 0, WMIN, EMAX)
    out = _step(f, k, 1, WMIN, EMAX)
    assert np.array_equal(ro, out)
    w, z, r = f.w, f.y, f.r
    np.testing.assert_array_equal(w[~train], 0.0)
    np.testing.assert_array_equal(r[~train], 0.0)
    np.testing.assert_array_equal(z[~train], eta_lin[~train])
    _check_rows("fold " + FOLD_IDS[FOLD_CASES.index((n, cap, pattern, ties, wts, presorted))], n, w, z, r, out, q, eta_lin, train,
                WMIN, unit=v is None or wts == "ones")
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
def test_one_stratum_and_unit_weights_are_the_plain_step_bit_for_bit(monkeypatch, n, cap):
    """w, z, r and out5 compared with ==: the new setter with both pointers NULL against cdh_glm_set_survival; explicit
    single-stratum ids plus weights of 1.0 (the segmented, weighted instantiations) against no strata and no weights (the
    plain ones); strata alone and weights alone likewise."""
    import test_gpu_cox as TG
    X, t, status, off, x = TG._data(n, "rounded", True, False)
    if cap != FULL:
        monkeypatch.setenv("CDH_COX_GRID", str(cap))
    y = np.c_[t, status]
    plain = cd.CDCoxLoss(y, X, off)
    want = _bits(plain, x)
    # the setter with both pointers NULL, on the same handle, is cdh_glm_set_survival
    cd.check(plain._L.cdh_glm_set_survival_strata(plain._h, _vp(t), _vp(status), _vp(off), None, None), plain._h)
    plain._synced = None
    _same(want, _bits(plain, x))
    plain.close()
    for g, v in ((np.full(n, 7), np.ones(n)), (np.full(n, -2 ** 31), None), (None, np.ones(n)), (np.zeros(n, dtype=np.int8), 2.5 * np.ones(n))):
        f = cd.CDCoxLoss(y, X, off, strata=g, weights=v)        # (constant weights normalise to ones exactly)
        np.testing.assert_array_equal(f.weights, np.ones(n))
        _same(want, _bits(f, x))
        f.close()


def test_repeatable_and_blind_to_folds_at_k_minus_one(monkeypatch):
    """The same step twice -- two identical steps on two handles, each read-only and applied -- and k = -1 with and without
    folds set: the same bits."""
    n, cap = 5 * T + 3, 2
    X, t, status, off, g, v, x = _data(n, cap, "cycling", "rounded", "uniform", True)
    got = []
    for folds in (False, False, True):
        f = _loss(monkeypatch, t, status, X, off, g, v, cap)
        if folds:
            f.set_folds(np.arange(n) % 3, 3)
        got.append(_bits(f, x))
        f.close()
    for other in got[1:]:
        _same(got[0], other)


# ---- the handle's other lives, and the refusals ----------------------------------------------------------------------------------
def test_set_survival_drops_strata_and_weights(monkeypatch):
    """cdh_glm_set_survival after the new setter: the getter returns zeros and ones and the step equals a fresh unstratified
    handle's bits; cdh_glm_set_labels drops them too, and the new setter brings them back on the same buffers."""
    n = T + 1
    X, t, status, off, g, v, x = _data(n, FULL, "wave", "distinct", "uniform", False)
    f = _loss(monkeypatch, t, status, X, off, g, v)
    with_strata = _bits(f, x)
    vn = f.weights
    L, h = f._L, f._h
    cd.check(L.cdh_glm_set_survival(h, _vp(t), _vp(status), _vp(off)), h)
    np.testing.assert_array_equal(f.strata, np.zeros(n, dtype=np.int32))
    np.testing.assert_array_equal(f.weights, np.ones(n))
    f._synced = None
    f._weighted = False
    fresh = cd.CDCoxLoss(np.c_[t, status], X, off)
    want = _bits(fresh, x)
    got = _bits(f, x)
    _same(want, got)
    assert not np.array_equal(got[2], with_strata[2])
    fresh.close()
    # getter: a NULL output is skipped, both NULL refused; not a Cox handle: refused
    gs, ws = np.full(n, 9, dtype=np.int32), np.full(n, 9.0)
    assert L.cdh_glm_get_survival_strata(h, _vp(gs), None) == OK and L.cdh_glm_get_survival_strata(h, None, _vp(ws)) == OK
    assert not gs.any() and np.all(ws == 1.0)
    assert L.cdh_glm_get_survival_strata(h, None, None) == BAD and L.cdh_glm_get_survival_strata(None, _vp(gs), None) == BAD
    labels = (np.random.default_rng(0).random(n) < 0.5).astype(np.float64)
    g32 = np.ascontiguousarray(g, dtype=np.int32)
    cd.check(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    cd.check(L.cdh_glm_set_labels(h, 0, _vp(labels)), h)
    assert L.cdh_glm_get_survival_strata(h, _vp(gs), None) == BAD
    cd.check(L.cdh_glm_set_survival(h, _vp(t), _vp(status), _vp(off)), h)      # after set_labels: still none
    assert L.cdh_glm_get_survival_strata(h, _vp(gs), _vp(ws)) == OK and not gs.any() and np.all(ws == 1.0)
    cd.check(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(status), _vp(off), _vp(g32), _vp(vn)), h)
    f._synced = None
    f._weighted = True
    _same(with_strata, _bits(f, x))
    f.close()


def test_refusals_leave_the_handle_unchanged(monkeypatch):
    n = 65
    X, t, status, off, g, v, x = _data(n, FULL, "lane", "distinct", "uniform", False)
    f = _loss(monkeypatch, t, status, X, off, g, v)
    cd.initialize_(f, x)
    before = _step(f, -1, 0)
    vn = f.weights
    L, h = f._L, f._h
    g32 = np.ascontiguousarray(g, dtype=np.int32)

    def refused(status_code, word=None):
        assert status_code == BAD
        assert len(L.cdh_last_error(h)) > 0
        if word is not None:
            assert word.encode() in L.cdh_last_error(h), L.cdh_last_error(h)

    for i, bad_v in ((7, 0.0), (0, -1.0), (64, np.nan), (11, np.inf)):
        bad = vn.copy()
        bad[i] = bad_v
        refused(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(status), _vp(off), _vp(g32), _vp(bad)), "weights[%d]" % i)
        refused(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(status), _vp(off), None, _vp(bad)), "weights[%d]" % i)
    bad = t.copy()
    bad[7] = np.nan
    refused(L.cdh_glm_set_survival_strata(h, _vp(bad), _vp(status), None, _vp(g32), _vp(vn)), "time[7]")
    bad = status.copy()
    bad[9] = 0.5
    refused(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(bad), None, _vp(g32), None), "status[9]")
    bad = off.copy()
    bad[3] = np.inf
    refused(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(status), _vp(bad), None, _vp(vn)), "offset[3]")
    refused(L.cdh_glm_set_survival_strata(h, _vp(t), _vp(np.zeros(n)), None, _vp(g32), _vp(vn)), "no row is an event")
    refused(L.cdh_glm_set_survival_strata(h, None, _vp(status), None, _vp(g32), _vp(vn)))
    refused(L.cdh_glm_set_survival_strata(h, _vp(t), None, None, _vp(g32), _vp(vn)))
    refused(L.cdh_glm_get_survival_strata(h, None, None))
    assert L.cdh_glm_set_survival_strata(None, _vp(t), _vp(status), None, _vp(g32), _vp(vn)) == BAD
    np.testing.assert_array_equal(f.time, t)
    np.testing.assert_array_equal(f.status, status)
    np.testing.assert_array_equal(f.offset, off)
    np.testing.assert_array_equal(f.strata, g)
    np.testing.assert_array_equal(f.weights, vn)
    assert np.array_equal(_step(f, -1, 0), before)               # the step's bits before and after the refused calls
    f.close()
