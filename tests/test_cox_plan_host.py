"""The Cox step without a GPU: the host arithmetic of cdh_glm_cox_irls and cdh_glm_set_survival (csrc/cox_plan.hpp) as a
stand-alone program under the host sanitizers and against its Python restatement (tests/_cox_plan.py) -- the plan, the
workgroups' contiguous runs, the scratch layout, the time order with its tie groups, the refusals of the data -- and the numpy
twin (tests/_cox_numpy.py): its O(n) cumulative-sum form against the O(n^2) definition, and its gradient against a central
difference of the negative log partial likelihood."""
import os
import re
import subprocess

import numpy as np
import pytest

import _cox_numpy as CX
import _cox_plan as CP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cox") / "cox_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cox_plan_main.cpp")], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def test_every_row_in_one_tile_every_tile_in_one_run(plan_exe):
    assert "cox_plan_main OK tile=1024" in _run(plan_exe)


LDS = (32, CP.TILE - 32, CP.TILE, CP.TILE + 32, 3 * CP.TILE + 32, 1024 * CP.TILE, 1024 * CP.TILE + 32, 2 ** 31 - 32)
CAPS = (1, 2, 7, 1024, 0, 5000)


def test_python_restatement_matches_the_header(plan_exe):
    cases = [(ld, cap) for ld in LDS for cap in CAPS]
    lines = _run(plan_exe, "plan", *[v for c in cases for v in c]).split("\n")
    for (ld, cap), line in zip(cases, lines):
        v = [int(x) for x in line.split()]
        pl, lay = CP.plan(ld, cap), CP.layout(ld)
        assert v[:4] == [pl["tiles"], pl["grid"], pl["records"], pl["longest"]], (ld, cap)
        g = pl["grid"]
        assert v[4:8] == [CP.run_first(pl["tiles"], g, b) for b in (0, 1, g - 1, g)], (ld, cap)
        assert v[8:] == [lay[k] for k in ("eT", "hA", "hB", "time", "sums", "doubles", "order", "first", "last", "ints")], (ld, cap)
        assert 1 <= g <= CP.MAX_GRID and g == min(pl["tiles"], CP.grid_cap(cap))


@pytest.fixture(scope="module")
def header_runs(plan_exe):
    """(ld, cap) -> (tiles, grid, the first tile of every run and one past the last), as cox_plan.hpp itself computes them."""
    cases = [(ld, cap) for ld in LDS for cap in CAPS]
    lines = _run(plan_exe, "runs", *[v for c in cases for v in c]).split("\n")
    return {c: np.array(line.split(), dtype=np.int64) for c, line in zip(cases, lines)}


@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("cap", CAPS)
def test_runs_partition_the_tiles(header_runs, ld, cap):
    """On the figures the header's own functions print: the runs are contiguous, non-empty, in order, start at tile 0 and end at
    the last tile -- every tile in exactly one workgroup's run -- the longest has `longest` tiles, and the tiles cover the rows;
    the Python restatement gives the same runs; the scratch sizes are the layout's."""
    v = header_runs[(ld, cap)]
    tiles, g, first = int(v[0]), int(v[1]), v[2:]
    pl = CP.plan(ld, cap)
    assert (tiles, g) == (pl["tiles"], pl["grid"]) and len(first) == g + 1 and 1 <= g <= CP.MAX_GRID
    assert first[0] == 0 and first[-1] == tiles and np.all(np.diff(first) >= 1) and np.diff(first).max() == pl["longest"]
    np.testing.assert_array_equal(first, np.arange(g + 1, dtype=np.int64) * tiles // g)
    assert (tiles - 1) * CP.TILE < ld <= tiles * CP.TILE                     # every row lies in exactly one tile
    lay = CP.layout(ld)
    assert lay["doubles"] == 4 * ld + 3 * CP.MAX_GRID and lay["ints"] == 3 * ld
    assert [lay[k] for k in ("eT", "hA", "hB", "time", "sums")] == [0, ld, 2 * ld, 3 * ld, 4 * ld]


def test_plan_header_holds_no_hip():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "cox_plan.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|hip[A-Z_]|threadIdx|blockIdx", code)
    k = open(os.path.join(CSRC, "cox_kernels.hpp")).read()
    for fn in ("CoxEta cox_eta(", "CoxRow cox_row("):
        body = k[k.index(fn):k.index("\n}\n", k.index(fn))]
        assert "#pragma clang fp contract(off)" in body and "asm" not in body
    code = re.sub(r"//[^\n]*", "", k)
    assert not re.search(r"atomic|cooperative|__threadfence|while\s*\(\s*(?:true|1)\s*\)|volatile", code)


# ---- the time order and the tie groups -----------------------------------------------------------------------------------------
ORDER_CASES = {
    "distinct": [3.5, 1.25, 2.0, 9.0, -1.0],
    "all equal": [2.0] * 6,
    "ties": [2.0, 1.0, 2.0, 1.0, 3.0, 2.0, 3.0],
    "sorted": [1.0, 2.0, 2.0, 4.0, 5.0],
    "reversed": [5.0, 4.0, 2.0, 2.0, 1.0],
    "one": [7.0],
    "forty": list(np.round(np.random.default_rng(3).exponential(1.0, 40), 1)),
}


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_order_and_group_bounds(plan_exe, name):
    t = np.array(ORDER_CASES[name])
    n, ld = len(t), CP.padded(len(t))
    got = [np.array(line.split(), dtype=np.int64) for line in _run(plan_exe, "order", *[repr(float(v)) for v in t]).split("\n")[:3]]
    order, first, last = CX.groups(t)
    for g, want in zip(got, (order, first, last)):
        assert g.shape == (ld,)
        np.testing.assert_array_equal(g[:n], want)
        np.testing.assert_array_equal(g[n:], np.arange(n, ld))              # the pad rows in place, each its own group
    ts = t[order]
    assert np.all(np.diff(ts) >= 0) and sorted(order.tolist()) == list(range(n))
    for s in range(n):
        grp = np.nonzero(ts == ts[s])[0]
        assert first[s] == grp[0] and last[s] == grp[-1]
        assert s == 0 or ts[s] != ts[s - 1] or order[s] > order[s - 1]      # stable


def test_data_refusals_name_the_row(plan_exe):
    def verdict(rows):
        return _run(plan_exe, "check", *[v for r in rows for v in r]).strip()

    good = [(1.0, 1, 0.0), (2.0, 0, 0.5), (2.0, 1, -0.5)]
    assert verdict(good) == "ok"
    assert verdict(good[:2] + [("nan", 1, 0.0)]) == "time[2] = nan is not finite"
    assert verdict([("inf", 1, 0.0)] + good).startswith("time[0] = inf")
    assert verdict(good[:1] + [(2.0, 0.5, 0.0)] + good[2:]).startswith("status[1] = 0.5 is neither")
    assert verdict(good + [(3.0, 1, "-inf")]).startswith("offset[3] = -inf")
    assert verdict([(1.0, 0, 0.0), (2.0, 0, 0.0)]).startswith("no row is an event")


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def _heavy_ties(n=300, seed=11, with_offset=True):
    X, t, status, off = CX.make_data(n, 4, seed, decimals=1, censor=0.3, with_offset=with_offset)
    rng = np.random.default_rng(seed + 1)
    eta_lin = X @ np.array([0.9, -0.7, 0.5, 0.0]) + 0.1 * rng.standard_normal(n)
    return X, t, status, off, eta_lin


def test_cumulative_form_agrees_with_the_definition():
    """n = 300, times rounded to one decimal (tie groups of up to tens of rows): the O(n) form against the fsum definition.
    Every scanned sum has positive terms, so a float64 cumulative sum of m terms is within (m - 1) U of exact, relatively;
    A and B add the error of S (and of S twice) in every term."""
    X, t, status, off, eta_lin = _heavy_ties()
    n = len(t)
    assert len(np.unique(t)) < n // 3
    for train in (None, np.arange(n) % 3 != 1):
        a = CX.rows(eta_lin, off, t, status, 1e-5, 50.0, train)
        b = CX.rows(eta_lin, off, t, status, 1e-5, 50.0, train, exact=True)
        ev = b["delta"] != 0.0
        eS = np.abs(a["S"] - b["S"])[ev] / b["S"][ev]
        pos = b["A"] > 0.0
        eA = np.abs(a["A"] - b["A"])[pos] / b["A"][pos]
        eB = np.abs(a["B"] - b["B"])[pos] / b["B"][pos]
        ew = np.abs(a["w_raw"] - b["w_raw"])[pos] / b["eA"][pos]
        print(f"twin O(n) vs fsum: S {eS.max() / U:.1f} A {eA.max() / U:.1f} B {eB.max() / U:.1f} w {ew.max() / U:.1f} ulp (bounds "
              f"{n + 8}, {2 * n + 16}, {3 * n + 16}, {5 * n + 64})")
        assert eS.max() <= (n + 8) * U and eA.max() <= (2 * n + 16) * U and eB.max() <= (3 * n + 16) * U
        assert ew.max() <= (5 * n + 64) * U
        assert np.array_equal(a["clamped"], b["clamped"]) and np.array_equal(a["capped"], b["capped"])
        before = t < t[b["delta"] != 0.0].min()
        tr = np.ones(n, dtype=bool) if train is None else train
        assert np.all(b["A"][before] == 0.0) and np.all(b["w"][before & tr] == 1e-5) and np.all(b["r"][before] == 0.0)
        if train is not None:
            assert np.all(b["w"][~train] == 0.0) and np.all(b["r"][~train] == 0.0) and np.array_equal(b["z"][~train], eta_lin[~train])
            # held-out rows leave the sums: the training rows' quantities are those of the training rows alone
            c = CX.rows(eta_lin[train], off[train], t[train], status[train], 1e-5, 50.0, None, exact=True)
            for k in ("S", "A", "B", "w", "r", "z"):
                np.testing.assert_array_equal(b[k][train], c[k])


def test_gradient_and_hessian_diagonal_against_differences():
    """-(delta - eA) is the gradient of the negative log partial likelihood in eta, and eA - e^2 B its Hessian's diagonal:
    central differences with step 1e-5 on eta of order one leave a truncation error of ~1e-10 and a rounding error of
    ~n U |npl| / step ~ 1e-9."""
    X, t, status, off, eta_lin = _heavy_ties(n=120, seed=5)
    eta = eta_lin + off
    q = CX.rows(eta_lin, off, t, status, 1e-300, 700.0, None, exact=True)
    g = -q["d"]
    step = 1e-5
    for i in (0, 7, 33, 64, 119, int(np.argmin(t)), int(np.argmax(t))):
        up, dn = eta.copy(), eta.copy()
        up[i] += step
        dn[i] -= step
        fd = (CX.npl(up, t, status) - CX.npl(dn, t, status)) / (2 * step)
        assert abs(fd - g[i]) <= 1e-7, (i, fd, g[i])
        gu = -CX.rows(up - off, off, t, status, 1e-300, 700.0, None, exact=True)["d"][i]
        gd = -CX.rows(dn - off, off, t, status, 1e-300, 700.0, None, exact=True)["d"][i]
        assert abs((gu - gd) / (2 * step) - q["w_raw"][i]) <= 1e-7, i
    assert abs(g.sum()) <= 1e-12 * len(t)                                   # the partial likelihood ignores a shift of eta
