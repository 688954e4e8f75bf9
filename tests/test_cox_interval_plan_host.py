"""Start-stop times of the Cox step without a GPU: cox_order_interval, cox_check_interval and the third pair of buffers of
cox_layout (csrc/cox_plan.hpp) as a stand-alone program under the host sanitizers (tests/cox_interval_plan_main.cpp) and
against the twin's searchsorted form; and the twin (tests/_cox_interval_numpy.py) against itself and against
tests/_cox_strata_numpy.py: its O(n) difference form against the fsum definition, its gradient against a central difference
of the negative log partial likelihood, starts below every stop against the strata twin bit for bit, and rows split at a cut
against the unsplit rows.

The two forms.  With U = 2^-53 and the fsum values taken as exact, to first order in U: a cumulative sum of at most n positive
terms is within n U of itself, so T and T2 are, and S = T - T2 adds one rounding: |dS| <= (n + 1) U (T + T2).  A hazard term
dv / S carries S's relative error, at most (n + 1) U rho with rho = max over the events of (T + T2) / S, and one division; the
cumulative sum P adds n U: |dP| <= ((n + 1) rho + n + 1) U P, and A = P(stop) - P(start) one more rounding:
|dA| <= ((n + 1) rho + n + 2) U (P(stop) + P(start)).  B's terms carry S twice and two divisions:
|dB| <= ((2n + 2) rho + n + 3) U (P_B(stop) + P_B(start)).  w_raw = evA - ev (ev B) has three products and a difference, each
rounded in both forms: |dw| <= ev |dA| + ev^2 |dB| + 8 U (evA + ev (ev B))."""
import math
import os
import subprocess

import numpy as np
import pytest

import _cox_interval_numpy as CI
import _cox_plan as CP
import _cox_strata_numpy as CS

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
T = CP.TILE


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coxi") / "cox_interval_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cox_interval_plan_main.cpp")], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


# ---- the header --------------------------------------------------------------------------------------------------------------
def test_orders_lookups_pads_and_the_third_pair_of_buffers(plan_exe):
    assert "cox_interval_plan_main OK tile=1024" in _run(plan_exe)


def test_layout_of_the_third_pair(plan_exe):
    lds = (32, T - 32, T, T + 32, 3 * T + 32, 2 ** 31 - 32)
    for ld, line in zip(lds, _run(plan_exe, "layout", *lds).split("\n")):
        assert [int(x) for x in line.split()] == [0, ld, 2 * ld, 3 * ld, 3 * ld + CP.MAX_GRID, 0, ld, 2 * ld, 2 * ld + CP.MAX_GRID], ld


def _brute(start, stop, g, order, order2, sfirst, slast):
    n = len(stop)
    lo, enter = np.full(n, -1), np.full(n, -1)
    for s in range(n):
        a, b = sfirst[s], slast[s]
        for q in range(b, a - 1, -1):
            if start[order2[q]] >= stop[order[s]]:
                lo[s] = q
        for q in range(a, b + 1):
            if stop[order[q]] <= start[order[s]]:
                enter[s] = q
    return lo, enter


def _strata(name, n, rng):
    if name == "one":
        return np.zeros(n, dtype=np.int64)
    if name == "two":
        return rng.integers(0, 2, n) * 9 - 4
    if name == "three":
        return rng.integers(0, 3, n)
    sizes = np.resize(np.arange(1, 8), n)                        # "cycling": sizes 1..7, ids descending in the caller's order
    return (1000 - np.repeat(np.arange(n), sizes)[:n]).astype(np.int64)


@pytest.mark.parametrize("name", ("one", "two", "three", "cycling"))
def test_order_against_the_brute_force_search(plan_exe, name):
    """n = 1, 2, 65 and 1025 (pads present: none is a multiple of 32), by the tests' recipe with distinct times and with
    rounded ones -- starts equal to other rows' stops, tied starts.  The first five vectors are cox_order_strata's
    (_cox_strata_numpy.groups), order2 the lexsort by (stratum, start), lo and enter a brute-force search inside the stratum and
    the twin's searchsorted form; the pads stay in place with lo = enter = -1."""
    for n in (1, 2, 65, 1025):
        for rounded in (False, True):
            rng = np.random.default_rng(31 * n + rounded)
            _, start, stop, status, _ = CI.make_data(n, 1, 17 * n + rounded, rounded=rounded)
            g = _strata(name, n, rng)
            args = [v for a, b, c in zip(start, stop, g) for v in (repr(float(a)), repr(float(b)), int(c))]
            got = [np.array(line.split(), dtype=np.int64) for line in _run(plan_exe, "order", *args).split("\n")[:9]]
            ld = CP.padded(n)
            assert ld > n and all(a.shape == (ld,) for a in got)
            order, first, last, sfirst, slast, order2, pos2, lo, enter = got
            for a, b in zip(got[:5], CS.groups(stop, g)):
                np.testing.assert_array_equal(a[:n], b)
            t_order, _, _, _, _, t_order2, t_lo, t_enter = CI.groups(start, stop, g)
            np.testing.assert_array_equal(order2[:n], t_order2)
            np.testing.assert_array_equal(order[pos2], order2)
            b_lo, b_enter = _brute(start, stop, g, order, order2, sfirst, slast)
            np.testing.assert_array_equal(lo[:n], b_lo, err_msg="%s n=%d" % (name, n))
            np.testing.assert_array_equal(enter[:n], b_enter, err_msg="%s n=%d" % (name, n))
            np.testing.assert_array_equal(lo[:n], t_lo)
            np.testing.assert_array_equal(enter[:n], t_enter)
            for a in (order, order2, pos2):
                np.testing.assert_array_equal(a[n:], np.arange(n, ld))
            assert np.all(lo[n:] == -1) and np.all(enter[n:] == -1)
            if rounded and n >= 65:                              # the ties the recipe is there for
                assert np.isin(start, stop[status == 1.0]).any() and len(np.unique(start)) < n
                assert (lo[:n] >= 0).any() and (enter[:n] >= 0).any()


def test_a_lookup_never_leaves_its_stratum(plan_exe):
    """Stratum 0 holds the smaller stops; a row of stratum 1 starts below every stop of its own stratum and above those of
    stratum 0 (enter = -1, not stratum 0's last position); a start equal to a stop; tied starts; stratum 2 has no event."""
    rows = [(0.0, 1.0, 0), (0.25, 1.25, 0), (1.5, 3.0, 1), (2.0, 4.0, 1), (0.5, 2.0, 1), (2.0, 2.5, 1), (0.0, 9.0, 2)]
    out = [[int(x) for x in line.split()] for line in _run(plan_exe, "order", *[v for r in rows for v in r]).split("\n")[:9]]
    order, order2, pos2, lo, enter = out[0][:7], out[5][:7], out[6][:7], out[7][:7], out[8][:7]
    assert order == [0, 1, 4, 5, 2, 3, 6] and order2 == [0, 1, 4, 2, 3, 5, 6] and pos2 == [0, 1, 2, 4, 5, 3, 6]
    assert lo == [-1, -1, 4, -1, -1, -1, -1]
    assert enter == [-1, -1, -1, 2, -1, 2, -1]


def test_start_refusals_name_the_row(plan_exe):
    def verdict(rows):
        return _run(plan_exe, "check", *[v for r in rows for v in r]).strip()

    good = [(0.0, 1.0), (-3.0, 2.0), (1.5, 2.0)]
    assert verdict(good) == "ok"
    assert verdict(good + [(2.0, 2.0)]).startswith("start[3] = 2 is not below stop[3] = 2")
    assert verdict([(5.0, 1.0)] + good).startswith("start[0] = 5 is not below stop[0] = 1")
    assert verdict(good[:1] + [("nan", 1.0)]).startswith("start[1] = nan is not finite")
    assert verdict(good[:2] + [("-inf", 1.0)]).startswith("start[2] = -inf is not finite")
    assert verdict(good + [("inf", 1.0)]).startswith("start[3] = inf is not finite")


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def _problem(n=300, seed=11, nstrata=3, rounded=True, zero=0.3):
    X, start, stop, status, off = CI.make_data(n, 4, seed, rounded=rounded, zero=zero)
    rng = np.random.default_rng(seed + 1)
    eta_lin = X @ CI.beta0(4) + 0.1 * rng.standard_normal(n)
    g = rng.integers(0, nstrata, n) * 7 - 3
    v = rng.uniform(0.25, 4.0, n)
    return X, start, stop, status, off, eta_lin, g, v


@pytest.mark.parametrize("n,rounded,zero", ((65, True, 0.3), (300, False, 0.0), (1025, True, 0.0), (2049, False, 0.3)))
def test_difference_form_agrees_with_the_definition(n, rounded, zero):
    """The O(n) difference form against the explicit risk sets, within the bounds of the module's docstring -- relative to
    T + T2 and P(stop) + P(start), the sizes the difference form reports."""
    X, start, stop, status, off, eta_lin, g, v = _problem(n, 11 + n, rounded=rounded, zero=zero)
    for train in (None, np.arange(n) % 3 != 1):
        a = CI.rows(eta_lin, off, start, stop, status, 1e-5, 1.5, train, strata=g, weights=v)
        b = CI.rows(eta_lin, off, start, stop, status, 1e-5, 1.5, train, exact=True, strata=g, weights=v)
        ev = b["delta"] != 0.0
        assert np.all(b["S"][ev] > 0.0)
        rho = float((a["S_size"][ev] / b["S"][ev]).max())
        cA, cB = (n + 1) * rho + n + 2, (2 * n + 2) * rho + n + 3
        bS = (n + 1) * U * a["S_size"]
        bA, bB = cA * U * a["A_size"], cB * U * a["B_size"]
        e = b["v"] * np.exp(np.minimum(eta_lin + off, 1.5))
        bw = e * bA + e * e * bB + 8 * U * (b["eA"] + e * (e * b["B"]))
        pos = a["A_size"] > 0.0
        mS = (np.abs(a["S"] - b["S"])[ev] / bS[ev]).max()
        mA = (np.abs(a["A"] - b["A"])[pos] / bA[pos]).max()
        mB = (np.abs(a["B"] - b["B"])[pos] / bB[pos]).max()
        mw = (np.abs(a["w_raw"] - b["w_raw"])[pos] / bw[pos]).max()
        unclamped = 1.0 - b["clamped"].sum() / (n if train is None else train.sum())
        print(f"interval twin O(n) vs fsum n={n}: rho {rho:.2f}; multiples of the bounds: S {mS:.3f} A {mA:.3f} B {mB:.3f} "
              f"w {mw:.3f}; unclamped {unclamped:.4f}")
        assert mS <= 1.0 and mA <= 1.0 and mB <= 1.0 and mw <= 1.0
        np.testing.assert_array_equal(a["A"][~pos], 0.0)
        np.testing.assert_array_equal(b["A"][~pos], 0.0)
        assert unclamped >= 0.5


def test_gradient_against_a_central_difference():
    """-(dv - evA) is the gradient of the interval negative log partial likelihood in eta (step 1e-5: truncation ~1e-10,
    rounding ~n U |npl| / step ~ 1e-9)."""
    X, start, stop, status, off, eta_lin, g, v = _problem(n=120, seed=5)
    n = len(stop)
    eta = eta_lin + off
    q = CI.rows(eta_lin, off, start, stop, status, 1e-300, 700.0, None, exact=True, strata=g, weights=v)
    grad = -q["d"]
    step = 1e-5
    for i in (0, 7, 33, 64, 119, int(np.argmin(stop)), int(np.argmax(stop)), int(np.argmax(start))):
        up, dn = eta.copy(), eta.copy()
        up[i] += step
        dn[i] -= step
        fd = (CI.npl(up, start, stop, status, g, v) - CI.npl(dn, start, stop, status, g, v)) / (2 * step)
        assert abs(fd - grad[i]) <= 1e-7 * max(1.0, v[i]), (i, fd, grad[i])
    for s in np.unique(g):                                      # a shift of eta inside ONE stratum changes nothing
        assert abs(grad[g == s].sum()) <= 1e-12 * n * v.max()
    gX, _ = CI.gradient(X, eta_lin, off, start, stop, status, None, g, v)
    np.testing.assert_array_equal(gX, -(X.T @ q["d"]) / n)


def test_starts_below_every_stop_are_the_strata_twin():
    """With every start below its stratum's smallest stop nobody enters late: lo = enter = -1 everywhere, and both forms are
    _cox_strata_numpy's, bit for bit; so is start=None."""
    X, _, stop, status, off, eta_lin, g, v = _problem()
    n = len(stop)
    start = np.full(n, stop.min() - 1.0) - np.random.default_rng(3).random(n)
    assert np.all(CI.groups(start, stop, g)[6] == -1) and np.all(CI.groups(start, stop, g)[7] == -1)
    for train in (None, np.arange(n) % 3 != 1):
        for exact in (False, True):
            want = CS.rows(eta_lin, off, stop, status, 1e-5, 50.0, train, exact=exact, strata=g, weights=v)
            for st in (start, None):
                got = CI.rows(eta_lin, off, st, stop, status, 1e-5, 50.0, train, exact=exact, strata=g, weights=v)
                for key in want:
                    np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    eta = eta_lin + off
    assert CI.npl(eta, start, stop, status, g, v) == CS.npl(eta, stop, status, g, v)


def test_splitting_rows_at_a_cut_changes_nothing():
    """(0, t] split at c into (0, c] censored and (c, t]: the same risk sets at every event time, so npl and the gradient in
    beta are unchanged up to the order of the sums: within 8 n U of the sums of the absolute terms."""
    X, _, stop, status, off, eta_lin, _, _ = _problem(n=200, seed=23, rounded=True)
    n = len(stop)
    beta = CI.beta0(4)
    for cut in (0.45, 0.5, float(np.median(stop))):              # 0.5 is an event time of the rounded recipe
        X2, start2, stop2, status2, off2, src = CI.split_rows(X, stop, status, off, cut)
        assert len(stop2) > n and np.all(start2 < stop2)
        if cut == 0.5:
            assert (stop[status == 1.0] == 0.5).any()
        a = CI.npl(X @ beta + off, np.zeros(n), stop, status)
        b = CI.npl(X2 @ beta + off2, start2, stop2, status2)
        assert abs(a - b) <= 8 * len(stop2) * U * (abs(a) + status.sum() * np.abs(X @ beta + off).max())
        qa = CI.rows(X @ beta, off, np.zeros(n), stop, status, 1e-300, 700.0, None, exact=True)
        qb = CI.rows(X2 @ beta, off2, start2, stop2, status2, 1e-300, 700.0, None, exact=True)
        ga, gb = X.T @ qa["d"], X2.T @ qb["d"]
        scale = np.abs(X).T @ (qa["delta"] + qa["eA"])
        assert np.all(np.abs(ga - gb) <= 8 * len(stop2) * U * scale), (ga, gb)
        # row by row: the pieces' d add up to the unsplit row's
        d = np.bincount(src, weights=qb["d"], minlength=n)
        assert np.max(np.abs(d - qa["d"]) / (qa["delta"] + qa["eA"] + 1e-300)) <= 8 * len(stop2) * U
