"""The case tables of tests/_glm_extremes.py without a GPU: every shape reaches the branch of the plan it is named for and puts
saturated entries where placement could matter; the clamp boundary keeps a margin no rounding of the device can cross;
numpy's exp, the reference of tests/test_gpu_glm_extremes.py, is held to mpmath on every argument the tables produce; the
twins' row formulas stay finite on the whole of both tables (dev = +inf exactly where y / mu overflows, never NaN); and the
twins' solves on the hard data sets converge to the figures the GPU cases are compared with, ordered or shuffled."""
import numpy as np
import pytest

import _cv_logistic_numpy as CL
import _glm_extremes as GX
import _glm_plan as GP
import _logistic_numpy as LG
import _poisson_numpy as PN


# ---- shapes and coverage -------------------------------------------------------------------------------------------------------
def test_shapes_reach_their_branches():
    for n, cap, branch in GX.SHAPES:
        GX.reaches(n, cap, branch)
    assert [s[0] for s in GX.SHAPES] == [33, GP.ROWS + 1, 2 * GP.ROWS + 1]


def _covers(cases, sat):
    T = len(sat)
    for n, cap, branch in GX.SHAPES:
        seen = np.zeros(T, dtype=bool)
        mine = [c for c in cases if c[0] == n]
        assert mine and len({c[3] for c in mine}) == len(mine)
        for _, _, _, start in mine:
            e = GX.entries(T, n, start)
            seen[e] = True
            assert sat[e[n - 1]] and (n <= GP.ROWS or sat[e[GP.ROWS]]), (n, start)
            held = GX.third(n)
            assert abs(held.sum() - n / 3) <= 1 and sat[e[held]].any() and sat[e[~held]].any(), (n, start)
        assert seen.all(), (n, np.flatnonzero(~seen))


def test_binomial_cases_cover_the_table_with_saturated_rows_where_placement_matters():
    eta, lab = GX.B_TABLE
    assert len(eta) == 3 * (2 * len(GX.B_ETAS) - 1) and set(lab) == {0.0, 1.0, 0.25}
    _covers(GX.B_CASES, np.abs(eta) >= GX.B_SAT)
    # the held-out third meets every label on both sides of zero, and the eta = 0 row with a label that makes it a miss
    zero_missed = False
    for n, _, _, start in GX.B_CASES:
        e = GX.entries(len(eta), n, start)
        held = GX.third(n)
        if n > GP.ROWS:
            for l in GX.B_LABELS:
                for s in (1.0, -1.0):
                    assert ((lab[e[held]] == l) & (np.sign(eta[e[held]]) == s) & (np.abs(eta[e[held]]) >= GX.B_SAT)).any(), (n, l, s)
        zero_missed |= bool(((eta[e[held]] == 0.0) & (lab[e[held]] > 0.0)).any())
    assert zero_missed
    assert CL.miss([1.0, 0.25, 0.0], [0.0, 0.0, 0.0]).tolist() == [1.0, 0.25, 0.0]       # eta = 0 predicts class 0


@pytest.mark.parametrize("eta_max", GX.P_ETA_MAX)
def test_poisson_cases_cover_the_table(eta_max):
    eta, cnt, place, lin, off = GX.P_TABLES[eta_max]
    T = len(eta)
    assert T == 3 * len(GX.P_COUNTS) * (len(GX.P_ETAS) + 2)
    _covers(GX.P_CASES[eta_max], np.abs(eta) >= GX.P_SAT)
    # the placements: through X the offset is zero, through the offset X beta is, and the cancellation comes to the listed value
    # wherever -800 + c is representable (the successor of 50 is not: that row comes to 50 itself and is not capped; the
    # successor of 700 is, and is)
    assert np.array_equal(lin + off, eta) and (off[place == 0] == 0.0).all() and (lin[place == 1] == 0.0).all()
    assert (lin[place == 2] == GX.CANCEL).all()
    same = eta[place == 2] == eta[place == 0]
    assert same.sum() == same.size - (len(GX.P_COUNTS) if eta_max == 50.0 else 0) and (eta[place == 2][~same] == eta_max).all()
    assert np.array_equal(eta[place == 0], eta[place == 1]) and np.array_equal(cnt[place == 0], cnt[place == 1])
    # every (X, offset) pair lies in two adjacent entries, and some case holds both
    both = np.zeros(T, dtype=bool)
    for n, _, _, start in GX.P_CASES[eta_max]:
        e = GX.entries(T, n, start)
        here = np.zeros(T, dtype=bool)
        here[e] = True
        both |= here & np.roll(here, -1)
    assert both[place == 0].all()
    # the row with dev == 0 and r == 0 exactly, the uncapped row at eta_max and the capped one above it
    w, z, r, nll, dev, cl, cap = PN.rows(cnt, lin, off, GX.WMIN, eta_max)
    i = np.flatnonzero((eta == 0.0) & (cnt == 1.0))
    assert len(i) == 3 and (dev[i] == 0.0).all() and (r[i] == 0.0).all()
    assert not cap[eta == eta_max].any() and cap[eta == np.nextafter(eta_max, np.inf)].all()
    assert cap.sum() == (eta > eta_max).sum() > 0 and (w[cap] == np.exp(eta_max)).all()


# ---- the clamp boundary ----------------------------------------------------------------------------------------------------------
def test_clamp_flags_keep_a_margin_the_device_cannot_cross():
    """The device's w_raw (mu) is within 64 ulp = 7e-15 relative of the twin's; a row's `clamped` can only differ where the
    twin's is within that of wmin.  Every table entry keeps 1e-9, the four boundary values included: two of them clamp."""
    eta, lab = GX.B_TABLE
    e = np.exp(-np.abs(eta))
    w_raw = e / ((1.0 + e) * (1.0 + e))
    assert np.min(np.abs(w_raw - GX.WMIN) / GX.WMIN) >= 1e-9
    near = np.array(GX.B_NEAR)
    e = np.exp(-near)
    w_raw = e / ((1.0 + e) * (1.0 + e))
    rel = (w_raw - GX.WMIN) / GX.WMIN
    print("clamp boundary", GX.B_EDGE, "w_raw / wmin - 1 at the four values", rel)
    assert (rel[:2] >= 1e-9).all() and (rel[2:] <= -1e-9).all() and (np.abs(rel) <= 2e-3).all()
    assert abs(GX.B_EDGE - np.log(1.0 / GX.WMIN)) < 1e-4 and 0.0 < GX.WMIN <= 0.25 and np.log2(GX.WMIN) == -17.0
    assert LG.rows(np.ones(4), near, GX.WMIN)[4].tolist() == [False, False, True, True]
    for em in GX.P_ETA_MAX:
        mu = np.exp(np.minimum(GX.P_TABLES[em][0], em))
        assert (np.abs(mu - GX.WMIN) >= 1e-9 * GX.WMIN).all()


# ---- numpy's exp against mpmath --------------------------------------------------------------------------------------------------
def test_numpy_exp_is_within_one_spacing_of_mpmath():
    """On every -|eta| of the binomial table and every capped eta of the Poisson tables: |np.exp - exp| <= 1 spacing of the
    result, a spacing of the subnormal range being 2^-1074.  That makes numpy a reference the GPU cases can use for the
    device's exp without mpmath there.  Measured when this was written: 0.50 spacings at the worst in either range, over 27
    arguments."""
    mp = pytest.importorskip("mpmath")
    args = set((-np.abs(GX.B_TABLE[0])).tolist())
    for em in GX.P_ETA_MAX:
        args |= set(np.minimum(GX.P_TABLES[em][0], em).tolist())
    worst = {}
    with mp.workprec(200):
        for x in sorted(args):
            v = float(np.exp(x))
            exact = mp.exp(mp.mpf(x))
            spacing = float(np.spacing(v)) if v >= 2.0 ** -1022 else GX.TINY
            d = float(abs(mp.mpf(v) - exact) / mp.mpf(spacing))
            rng = "subnormal" if v < 2.0 ** -1022 else "normal"
            worst[rng] = max(worst.get(rng, 0.0), d)
            assert d <= 1.0, (x, v, d)
    print("np.exp against mpmath at 200 bits, worst distance in spacings:", worst, "over", len(args), "arguments")
    assert set(worst) == {"normal", "subnormal"}


# ---- the twins on the whole tables -----------------------------------------------------------------------------------------------
def test_binomial_twin_is_finite_on_the_whole_table():
    eta, lab = GX.B_TABLE
    w, z, r, nll, cl = LG.rows(lab, eta, GX.WMIN)
    for v in (w, z, r, nll):
        assert np.isfinite(v).all()
    big = np.abs(eta) >= 40.0
    assert (w[big] == GX.WMIN).all() and cl[big].all() and not cl[np.abs(eta) <= 1.0].any()
    one = (1.0 + np.exp(-np.abs(eta))) == 1.0
    assert np.array_equal(one, np.abs(eta) >= 37.5)           # 1 + e rounds to 1 from 36.7368 on: 36.7 is below, 37.5 above
    wrong = one & (((lab == 0.0) & (eta > 0.0)) | ((lab == 1.0) & (eta < 0.0)))
    assert (r[wrong] == -np.sign(eta[wrong]) / GX.WMIN).all() and (nll[wrong] == np.abs(eta[wrong])).all()
    right = one & (((lab == 1.0) & (eta > 0.0)) | ((lab == 0.0) & (eta < 0.0)))
    assert (r[right] == np.sign(eta[right]) * np.exp(-np.abs(eta[right])) / GX.WMIN).all()
    assert (r[right & (np.abs(eta) <= 745.13)] != 0.0).all() and (r[right & (np.abs(eta) >= 746.0)] == 0.0).all()
    down = right & (eta < 0.0)
    assert (nll[down] == np.exp(eta[down])).all() and (nll[right & (eta > 0.0)] == 0.0).all()


def overflows(cnt, mu):
    with np.errstate(over="ignore", divide="ignore"):
        return (cnt > 0.0) & np.isinf(np.where(cnt > 0.0, cnt, 1.0) / mu)


@pytest.mark.parametrize("eta_max", GX.P_ETA_MAX)
def test_poisson_twin_is_finite_on_the_whole_table_but_for_the_deviance(eta_max):
    eta, cnt, place, lin, off = GX.P_TABLES[eta_max]
    w, z, r, nll, dev, cl, cap = PN.rows(cnt, lin, off, GX.WMIN, eta_max)
    for v in (w, z, r, nll):
        assert np.isfinite(v).all()
    assert not np.isnan(dev).any()
    mu = np.exp(np.minimum(eta, eta_max))
    inf = overflows(cnt, mu)
    assert np.array_equal(dev == np.inf, inf) and np.isfinite(dev[~inf]).all() and 0 < inf.sum() < len(eta)
    assert inf[(cnt == 1.0) & (eta <= -745.0)].all() and inf[(cnt == 1e300) & (eta == -20.0)].all()
    assert not inf[(cnt == 3.0) & (eta == -700.0)].any()
    zero = cnt == 0.0
    assert (dev[zero] == 2.0 * mu[zero]).all() and (r[zero & cl] == -mu[zero & cl] / GX.WMIN).all()
    assert (w[~cl] == mu[~cl]).all()


# ---- the hard solves -------------------------------------------------------------------------------------------------------------
# name -> (rounds, clamped rows at the solution, capped rows, converged): the figures the data sets were chosen for
FIGURES = {"separable-0.01": (13, 91, 0, True), "separable-0.002": (21, 195, 0, True), "exposures": (7, 60, 0, True),
           "exposures-b": (6, 60, 0, True), "capped": (3, 59, 23, False), "capped-b": (3, 58, 42, False)}


@pytest.mark.parametrize("name", list(GX.SOLVES))
def test_twin_solves_on_the_hard_data(name):
    """Ordered and shuffled sweeps agree to 1e-11 (measured: 3.6e-12 at the worst), so the device may differ from either by
    the project's 1e-10; no row's clamped or capped flag at the solution is within 1e-6 relative of flipping; F's largest
    rise is either rounding (<= 1e-12) or plain (the capped solves), so `monotone` has one answer; the converged solves
    satisfy the KKT conditions of F at 1e-11."""
    a, b = GX.twin_solve(name), GX.twin_solve(name, True)
    assert (a["rounds"], a["clamped"], a["capped"], a["converged"]) == FIGURES[name]
    assert (b["rounds"], b["clamped"], b["capped"], b["converged"]) == FIGURES[name]
    d = max(float(np.max(np.abs(a["beta"] - b["beta"]))), abs(a["b0"] - b["b0"]))
    wmin, emax = a["irls"]["wmin"], a["irls"]["etaMax"]
    if a["family"] == "binomial":
        e = np.exp(-np.abs(a["eta"]))
        margin = float(np.min(np.abs(e / ((1.0 + e) * (1.0 + e)) - wmin) / wmin))
        kkt = LG.kkt(a["X"], a["y"], a["beta"], a["lam"])[:2]
        F = LG.objective(a["X"], a["y"], a["beta"], a["lam"])
    else:
        full = a["eta"] + a["o"]
        margin = float(min(np.min(np.abs(np.exp(np.minimum(full, emax)) - wmin) / wmin), np.min(np.abs(full - emax) / emax)))
        kkt = PN.kkt(a["X"], a["y"], a["o"], a["beta"], a["lam"], None, a["b0"])
        kkt = kkt if a["icpt"] else kkt[:2]
        F = PN.objective(a["X"], a["y"], a["o"], a["beta"], a["lam"], None, a["b0"])
    print(f"twin [{name}]: rounds {a['rounds']} clamped {a['clamped']} capped {a['capped']} max|eta| {np.max(np.abs(a['eta'])):.1f} "
          f"ordered - shuffled {d:.1e} flag margin {margin:.1e} rise {a['rise']:.1e} F {F:.3f} KKT {max(kkt):.1e}")
    assert d <= 1e-11 and margin >= 1e-6
    for t in (a, b):
        assert t["rise"] <= 1e-12 or t["rise"] > 1e-6 * max(1.0, abs(F))
        assert t["monotone"] == t["converged"]               # (here: the capped solves rise and stop at maxIter = 3)
    if a["converged"]:
        assert max(kkt) <= 1e-11 and np.count_nonzero(a["beta"]) >= 3
