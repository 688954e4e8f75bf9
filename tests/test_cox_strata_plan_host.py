"""Strata and observation weights of the Cox step without a GPU: cox_order_strata, the second pair of buffers of cox_layout
and cox_check's refusal of the weights (csrc/cox_plan.hpp) as a stand-alone program under the host sanitizers
(tests/cox_strata_plan_main.cpp) and against the twin's np.lexsort form; and the twin (tests/_cox_strata_numpy.py) against
itself and against tests/_cox_numpy.py: its O(n) form against the fsum definition, its gradient against a central difference
of the negative log partial likelihood, one stratum with unit weights and every stratum run alone against the unstratified
twin bit for bit, integer weights against replicated rows."""
import math
import os
import subprocess

import numpy as np
import pytest

import _cox_numpy as CX
import _cox_plan as CP
import _cox_strata_numpy as CS

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
T = CP.TILE


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coxs") / "cox_strata_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cox_strata_plan_main.cpp")], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


# ---- the header --------------------------------------------------------------------------------------------------------------
def test_orders_bounds_pads_and_the_second_pair_of_buffers(plan_exe):
    assert "cox_strata_plan_main OK tile=1024" in _run(plan_exe)


def test_layout_of_the_second_pair(plan_exe):
    lds = (32, T - 32, T, T + 32, 3 * T + 32, 2 ** 31 - 32)
    for ld, line in zip(lds, _run(plan_exe, "layout", *lds).split("\n")):
        assert [int(x) for x in line.split()] == [0, ld, 2 * ld, 3 * ld, 3 * ld + 2 * CP.MAX_GRID, 0, ld], ld


def _pattern(name, n, rng):
    if name == "one":
        return np.zeros(n, dtype=np.int64)
    if name == "two":
        return rng.integers(0, 2, n)
    if name == "cycling":                                        # sizes 1..7 cycling, ids descending in the caller's order
        sizes = np.resize(np.arange(1, 8), n)
        return (1000 - np.repeat(np.arange(n), sizes)[:n]).astype(np.int64)
    if name == "own":
        return rng.permutation(n).astype(np.int64)
    return rng.choice(np.array([-2 ** 31, -5, 0, 2 ** 31 - 1], dtype=np.int64), n)      # "extreme"


ORDER_NS = list(range(1, 41)) + [63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 2100]


@pytest.mark.parametrize("name", ("one", "two", "cycling", "own", "extreme"))
def test_order_against_the_lexsort_form(plan_exe, name):
    """order, first, last, sfirst and slast for n = 1 .. 40, around the wave, the tile and two tiles and at 2100, times with
    ties (rounded) and without; the pads in place and one stratum; one stratum gives cox_order's vectors (_cox_numpy.groups)."""
    for n in ORDER_NS:
        for ties in (False, True):
            rng = np.random.default_rng(100 * n + ties)
            t = rng.exponential(1.0, n)
            if ties:
                t = np.round(t, 1)
            g = _pattern(name, n, rng)
            args = [v for a, b in zip(t, g) for v in (repr(float(a)), int(b))]
            got = [np.array(line.split(), dtype=np.int64) for line in _run(plan_exe, "order", *args).split("\n")[:5]]
            want = CS.groups(t, g)
            ld = CP.padded(n)
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.shape == (ld,)
                np.testing.assert_array_equal(a[:n], b, err_msg="%s n=%d vector %d" % (name, n, k))
            for a in got[:3]:
                np.testing.assert_array_equal(a[n:], np.arange(n, ld))
            np.testing.assert_array_equal(got[3][n:], n)
            np.testing.assert_array_equal(got[4][n:], ld - 1)
            if name == "one":
                for a, b in zip(got[:3], CX.groups(t)):
                    np.testing.assert_array_equal(a[:n], b)
                assert np.all(got[3][:n] == 0) and np.all(got[4][:n] == n - 1)


def test_data_refusals_name_the_row(plan_exe):
    def verdict(rows):
        return _run(plan_exe, "check", *[v for r in rows for v in r]).strip()

    good = [(1.0, 1, 0.0, 1.0), (2.0, 0, 0.5, 0.25), (2.0, 1, -0.5, 4.0)]
    assert verdict(good) == "ok"
    assert verdict(good[:2] + [(3.0, 1, 0.0, 0.0)]).startswith("weights[2] = 0 is not finite and > 0")
    assert verdict([(1.0, 1, 0.0, -1.0)] + good).startswith("weights[0] = -1")
    assert verdict(good[:1] + [(2.0, 0, 0.0, "nan")] + good[2:]).startswith("weights[1] = nan")
    assert verdict(good + [(3.0, 1, 0.0, "inf")]).startswith("weights[3] = inf")
    # the earlier refusals stand, in their order
    assert verdict(good[:2] + [("nan", 1, 0.0, 1.0)]) == "time[2] = nan is not finite"
    assert verdict(good[:1] + [(2.0, 0.5, 0.0, 1.0)]).startswith("status[1] = 0.5 is neither")
    assert verdict(good + [(3.0, 1, "-inf", 1.0)]).startswith("offset[3] = -inf")
    assert verdict([(1.0, 0, 0.0, 1.0), (2.0, 0, 0.0, 2.0)]).startswith("no row is an event")


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def _problem(n=300, seed=11, nstrata=3, scale=False):
    X, t, status, off = CX.make_data(n, 4, seed, decimals=1, censor=0.3, with_offset=True)
    rng = np.random.default_rng(seed + 1)
    eta_lin = X @ np.array([0.9, -0.7, 0.5, 0.0]) + 0.1 * rng.standard_normal(n)
    g = rng.integers(0, nstrata, n) * 7 - 3
    v = rng.uniform(0.25, 4.0, n)
    if scale:
        off = off + 30.0 * (g == g.max())
    return X, t, status, off, eta_lin, g, v


@pytest.mark.parametrize("scale", (False, True))
def test_cumulative_form_agrees_with_the_definition(scale):
    """The O(n) form against the fsum definition within the bounds of tests/test_gpu_cox.py's docstring, RELATIVE TO THE
    STRATUM'S OWN sums -- also where one stratum's sums are e^30 times another's."""
    X, t, status, off, eta_lin, g, v = _problem(scale=scale)
    n = len(t)
    for train in (None, np.arange(n) % 3 != 1):
        a = CS.rows(eta_lin, off, t, status, 1e-5, 50.0, train, strata=g, weights=v)
        b = CS.rows(eta_lin, off, t, status, 1e-5, 50.0, train, exact=True, strata=g, weights=v)
        ev = b["delta"] != 0.0
        pos = b["A"] > 0.0
        eS = np.abs(a["S"] - b["S"])[ev] / b["S"][ev]
        eA = np.abs(a["A"] - b["A"])[pos] / b["A"][pos]
        eB = np.abs(a["B"] - b["B"])[pos] / b["B"][pos]
        ew = np.abs(a["w_raw"] - b["w_raw"])[pos] / b["eA"][pos]
        print(f"strata twin O(n) vs fsum (scale={scale}): S {eS.max() / U:.1f} A {eA.max() / U:.1f} B {eB.max() / U:.1f} "
              f"w {ew.max() / U:.1f} ulp")
        assert eS.max() <= (n + 8) * U and eA.max() <= (2 * n + 16) * U and eB.max() <= (3 * n + 16) * U
        assert ew.max() <= (5 * n + 64) * U
        assert np.array_equal(a["clamped"], b["clamped"])


def test_gradient_against_a_central_difference():
    """-(dv - evA) is the gradient of the weighted stratified negative log partial likelihood in eta (step 1e-5: truncation
    ~1e-10, rounding ~n U |npl| / step ~ 1e-9)."""
    X, t, status, off, eta_lin, g, v = _problem(n=120, seed=5)
    eta = eta_lin + off
    q = CS.rows(eta_lin, off, t, status, 1e-300, 700.0, None, exact=True, strata=g, weights=v)
    grad = -q["d"]
    step = 1e-5
    for i in (0, 7, 33, 64, 119, int(np.argmin(t)), int(np.argmax(t))):
        up, dn = eta.copy(), eta.copy()
        up[i] += step
        dn[i] -= step
        fd = (CS.npl(up, t, status, g, v) - CS.npl(dn, t, status, g, v)) / (2 * step)
        assert abs(fd - grad[i]) <= 1e-7 * max(1.0, v[i]), (i, fd, grad[i])
    for s in np.unique(g):                                      # a shift of eta inside ONE stratum changes nothing
        assert abs(grad[g == s].sum()) <= 1e-12 * len(t) * v.max()
    gX, _ = CS.gradient(X, eta_lin, off, t, status, None, g, v)
    np.testing.assert_array_equal(gX, -(X.T @ q["d"]) / len(t))


def test_one_stratum_and_unit_weights_are_the_unstratified_twin():
    X, t, status, off, eta_lin, g, v = _problem()
    n = len(t)
    for train in (None, np.arange(n) % 3 != 1):
        a = CX.rows(eta_lin, off, t, status, 1e-5, 50.0, train, exact=True)
        for strata, weights in ((None, None), (np.full(n, 9), np.ones(n)), (np.full(n, -4), None), (None, np.ones(n))):
            b = CS.rows(eta_lin, off, t, status, 1e-5, 50.0, train, exact=True, strata=strata, weights=weights)
            for key in a:
                np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        a = CX.rows(eta_lin, off, t, status, 1e-5, 50.0, train)
        b = CS.rows(eta_lin, off, t, status, 1e-5, 50.0, train, strata=np.zeros(n, dtype=int), weights=np.ones(n))
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_a_stratified_problem_is_its_strata_run_alone():
    """Unit weights: the exact rows of a stratified problem are, stratum by stratum, the unstratified twin's on that stratum's
    rows alone, bit for bit, and the nll is the sum of theirs."""
    X, t, status, off, eta_lin, g, _ = _problem(scale=True)
    q = CS.rows(eta_lin, off, t, status, 1e-5, 50.0, None, exact=True, strata=g)
    parts = []
    for s in np.unique(g):
        m = g == s
        alone = CX.rows(eta_lin[m], off[m], t[m], status[m], 1e-5, 50.0, None, exact=True)
        for key in ("w", "z", "r", "nll", "S", "A", "B", "clamped"):
            np.testing.assert_array_equal(q[key][m], alone[key], err_msg=key)
        parts.append(alone["nll"])
    assert math.fsum(q["nll"]) == math.fsum(np.concatenate(parts))
    eta = eta_lin + off
    total = sum(CX.npl(eta[g == s], t[g == s], status[g == s]) for s in np.unique(g))
    assert abs(CS.npl(eta, t, status, g) - total) <= 4 * U * abs(total)


def test_integer_weights_reproduce_replicated_rows():
    """v in {1, 2, 3}: the gradient X'(dv - evA) and the nll are those of the problem with every row repeated v times (ties
    are Breslow's, so the copies share a risk set); the diagonal is not."""
    X, t, status, off, eta_lin, g, _ = _problem(n=90, seed=3)
    n = len(t)
    v = np.random.default_rng(8).integers(1, 4, n)
    rep = np.repeat(np.arange(n), v)
    a = CS.rows(eta_lin, off, t, status, 1e-300, 700.0, None, exact=True, strata=g, weights=v.astype(float))
    b = CS.rows(eta_lin[rep], off[rep], t[rep], status[rep], 1e-300, 700.0, None, exact=True, strata=g[rep])
    d_rep = np.bincount(rep, weights=b["d"], minlength=n)
    scale = a["delta"] + a["eA"]
    assert np.max(np.abs(a["d"] - d_rep) / np.maximum(scale, 1e-300)) <= 16 * U * v.max()
    np.testing.assert_allclose(a["S"], b["S"][np.cumsum(v) - 1], rtol=4 * U * n, atol=0.0)
    na, nb = math.fsum(a["nll"]), math.fsum(b["nll"])
    assert abs(na - nb) <= 8 * n * U * math.fsum(np.abs(b["nll"]))
    assert np.max(np.abs(a["w_raw"] - np.bincount(rep, weights=b["w_raw"], minlength=n))) > 1e-6
