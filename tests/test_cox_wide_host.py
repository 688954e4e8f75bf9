"""The references of tests/test_gpu_cox_runs.py without a GPU.

1. The wide twin (tests/_cox_wide_numpy.py: longdouble cumulative sums, rounded once) against the fsum definitions
   (`scans_exact` of the three twins) at the shapes the other host tests use.  Reference against reference, U = 2^-53:
       S    within 1 ulp: the wide sum rounds once, fsum is correctly rounded, and the wide sum's own error before its rounding
            (n 2^-64, for the interval form relative to T + T2) is far below an ulp at these n;
       A    within 3 U A, B within 4 U B: the definition's terms dv / S and (dv / S) / S carry the rounding of S and one or two
            rounded divisions that the wide form does not round, and each form rounds its sum once.
2. The closed forms of the GPU test's exact leg (tests/_cox_runs_cases.exact_problem) against the strata and the interval
   twins, both forms of each, at n = 3T + 37 with rows in random order: S, A, B, w, r, z and the clamps, bit for bit.
3. Every shape assert of every GPU case: the runs, the strata's boundaries against them, the tie groups across run edges, the
   lookups of the strata that nobody enters late.  Pure tests/_cox_plan.py arithmetic."""
import numpy as np
import pytest

import _cox_interval_numpy as CI
import _cox_numpy as CX
import _cox_plan as CP
import _cox_runs_cases as RC
import _cox_strata_numpy as CS
import _cox_wide_numpy as CW
import test_cox_interval_plan_host as HI
import test_cox_plan_host as HP
import test_cox_strata_plan_host as HS

U = 2.0 ** -53
T = CP.TILE


# ---- 1. the wide twin against the definitions ------------------------------------------------------------------------------------
def _pin(tag, q, b):
    """q: the wide rows, b: the fsum rows."""
    ev = b["delta"] != 0.0
    pos = b["A"] > 0.0
    assert ev.any() and pos.any()
    mS = (np.abs(q["S"] - b["S"])[ev] / np.spacing(np.minimum(q["S"], b["S"])[ev])).max()
    mA = (np.abs(q["A"] - b["A"])[pos] / (3 * U * b["A"][pos])).max()
    mB = (np.abs(q["B"] - b["B"])[pos] / (4 * U * b["B"][pos])).max()
    print(f"wide twin vs fsum, {tag}: S {mS:.0f} ulp; multiples of the bounds: A {mA:.3f} B {mB:.3f}")
    assert mS <= 1.0 and mA <= 1.0 and mB <= 1.0
    np.testing.assert_array_equal(q["A"][~pos], 0.0)
    np.testing.assert_array_equal(q["B"][~pos], 0.0)
    for key in ("capped", "delta", "e", "v"):
        if key in b:
            np.testing.assert_array_equal(q[key], b[key], err_msg=key)


def _trains(n):
    return (None, np.arange(n) % 3 != 1)


def test_wide_twin_agrees_with_the_definition_plain():
    X, t, status, off, eta_lin = HP._heavy_ties()
    for train in _trains(len(t)):
        _pin("plain n=300", CW.rows(eta_lin, off, t, status, 1e-5, 50.0, train),
             CX.rows(eta_lin, off, t, status, 1e-5, 50.0, train, exact=True))
    q = CW.rows(eta_lin, None, t, status, 1e-5, 50.0)            # the dict is _cox_numpy.rows', key for key
    assert set(CX.rows(eta_lin, None, t, status, 1e-5, 50.0)) <= set(q)


@pytest.mark.parametrize("scale", (False, True))
def test_wide_twin_agrees_with_the_definition_strata(scale):
    X, t, status, off, eta_lin, g, v = HS._problem(scale=scale)
    for train in _trains(len(t)):
        _pin(f"strata n=300 scale={scale}", CW.rows(eta_lin, off, t, status, 1e-5, 50.0, train, g, v),
             CS.rows(eta_lin, off, t, status, 1e-5, 50.0, train, exact=True, strata=g, weights=v))


@pytest.mark.parametrize("n,rounded,zero", ((65, True, 0.3), (300, False, 0.0), (1025, True, 0.0), (2049, False, 0.3)))
def test_wide_twin_agrees_with_the_definition_interval(n, rounded, zero):
    X, start, stop, status, off, eta_lin, g, v = HI._problem(n, 11 + n, rounded=rounded, zero=zero)
    for train in _trains(n):
        _pin(f"interval n={n}", CW.rows(eta_lin, off, stop, status, 1e-5, 1.5, train, g, v, start),
             CI.rows(eta_lin, off, start, stop, status, 1e-5, 1.5, train, exact=True, strata=g, weights=v))


def test_wide_twin_without_starts_is_its_strata_form():
    """Starts below every stop: nothing is subtracted, and the interval form gives the strata form's bits."""
    X, _, stop, status, off, eta_lin, g, v = HI._problem()
    start = np.full(len(stop), stop.min() - 1.0)
    a = CW.rows(eta_lin, off, stop, status, 1e-5, 50.0, None, g, v)
    b = CW.rows(eta_lin, off, stop, status, 1e-5, 50.0, None, g, v, start)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# ---- 2. the closed forms of the exact leg ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("late", ("none", "half", "all"))
def test_closed_forms_are_the_twins_bit_for_bit(late):
    n = 3 * T + 37
    sizes = np.array([2048, 512, 256, 128, 64, 32, 16, 8, 4, 2, 2, 1, 32, 4])
    assert sizes.sum() == n
    late_s = {"none": np.zeros(len(sizes), dtype=bool), "half": (np.arange(len(sizes)) % 2 == 1) & (sizes >= 2),
              "all": sizes >= 2}[late]
    c = RC.exact_problem(sizes, late_s, np.random.default_rng(n).permutation(n))
    assert (c["start"] is None) == (late == "none")
    # who clamps: the late half of every late stratum, and the rows whose S at the event is 1 (size 1; size 2, late: its early row)
    assert c["out2"] == (sizes[late_s] // 2).sum() + (sizes == 1).sum() + (late_s & (sizes == 2)).sum()
    assert c["out2"] == {"none": 1, "half": 345, "all": (n - 1) // 2 + 3}[late]      # one row in 3109; a ninth; half
    zero, ones = np.zeros(n), np.ones(n)
    forms = [lambda exact: CI.rows(zero, None, c["start"], c["time"], c["status"], RC.WMIN, RC.EMAX, None, exact=exact,
                                   strata=c["g"], weights=ones)]
    if late == "none":                                           # the strata twin too, and the interval twin with every start at 0
        forms.append(lambda exact: CS.rows(zero, None, c["time"], c["status"], RC.WMIN, RC.EMAX, None, exact=exact,
                                           strata=c["g"], weights=ones))
        forms.append(lambda exact: CI.rows(zero, None, zero, c["time"], c["status"], RC.WMIN, RC.EMAX, None, exact=exact,
                                           strata=c["g"], weights=ones))
    forms.append(lambda exact: CW.rows(zero, None, c["time"], c["status"], RC.WMIN, RC.EMAX, None, c["g"], ones, c["start"]))
    for form in forms:
        for exact in (False, True):
            q = form(exact)
            for key in ("S", "A", "B", "w", "r", "clamped"):
                np.testing.assert_array_equal(q[key], c[key], err_msg=key)
            np.testing.assert_array_equal(q["z"], c["r"])
            assert not q["capped"].any() and q["delta"].sum() == c["out4"] == len(sizes)
            np.testing.assert_array_equal(np.sort(q["S"][q["delta"] != 0.0]), np.sort(c["S_event"]))


# ---- 3. the shapes of the GPU cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_shapes(name):
    edges = RC.assert_shape(name)
    assert np.all(np.diff(edges) > 0) and edges[-2] < RC.SHAPES[name]      # the last run holds real rows
    if name == "R1024":
        a, b = RC.held_stretch(name)
        assert 0 < a < b < RC.SHAPES[name]


@pytest.mark.parametrize("name", list(RC.SHAPES))
@pytest.mark.parametrize("interval", (False, True), ids=("strata", "interval"))
def test_exact_cases_are_arranged_as_they_say(name, interval):
    """exact_case asserts the arrangement itself; here too: the sorted order puts the strata where the sizes say, the early
    strata of the interval chain have every lookup -1, the late ones have lo and enter at work."""
    c = RC.exact_case(name, interval)
    n = RC.SHAPES[name]
    assert len(c["time"]) == n and c["out4"] == len(c["sizes"])
    order, first, last, sfirst, slast = CS.groups(c["time"], c["g"])
    ends = np.cumsum(c["sizes"])
    np.testing.assert_array_equal(np.unique(sfirst), ends - c["sizes"])
    np.testing.assert_array_equal(first, np.arange(n))          # distinct times inside every stratum
    np.testing.assert_array_equal(c["time"][order][sfirst], 1.0)
    np.testing.assert_array_equal(c["status"][order][sfirst], 1.0)
    if RC.PRESORTED[name]:
        np.testing.assert_array_equal(order, np.arange(n))
    else:
        assert np.any(order != np.arange(n))
    if interval:
        lo, enter = CI.groups(c["start"], c["time"], c["g"])[6:]
        late = np.repeat(c["late_strata"], c["sizes"])          # per sorted position
        assert late.any() and (~late).any()
        assert np.all(lo[~late] == -1) and np.all(enter[~late] == -1)
        m = np.repeat(c["sizes"], c["sizes"])
        event = sfirst == np.arange(n)
        np.testing.assert_array_equal(lo[late & event], (sfirst + m // 2)[late & event])
        assert np.all(lo[late & ~event] == -1)
        np.testing.assert_array_equal(enter[late], np.where(np.arange(n) - sfirst >= m // 2, sfirst, -1)[late])
    else:
        assert c["start"] is None


@pytest.mark.parametrize("name", list(RC.SHAPES))
@pytest.mark.parametrize("chain", ("plain", "strata", "interval"))
def test_random_cases_are_arranged_as_they_say(name, chain):
    c = RC.random_case(name, chain)
    order, first, last, sfirst, slast = CS.groups(c["time"], c["g"])
    RC.assert_random_arrangement(name, chain, first, sfirst, slast)
    assert (c["g"] is None) == (c["v"] is None) == (chain == "plain") and (c["start"] is not None) == (chain == "interval")
    if chain == "interval":
        assert np.all(c["start"] < c["time"]) and np.isin(c["start"], c["time"][c["status"] == 1.0]).any()
        lo, enter = CI.groups(c["start"], c["time"], c["g"])[6:]
        assert (lo >= 0).any() and (enter >= 0).any()
    if chain != "plain":
        assert c["g"].min() < 0 and 0.25 <= c["v"].min() and c["v"].max() <= 4.0
        assert set(np.unique(np.diff(np.r_[np.unique(sfirst), len(first)]))) <= {1 << k for k in range(14)}
