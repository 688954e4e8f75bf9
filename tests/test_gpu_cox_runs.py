"""The Cox step at the full grid, where the scan over the RUNS works.  The chain of scans has three levels: a lane scans its four
positions, cox_block_excl the workgroup, and k_cox_offsets -- one workgroup -- turns the per-run records (sum since the last
head, head seen) into the offset every run starts from.  tests/test_gpu_cox.py, test_gpu_cox_strata.py and
test_gpu_cox_interval.py stop at 3 runs at the full grid and 2 with the grid capped: with 4 runs or fewer every run sits in
ONE lane of k_cox_offsets, cox_block_excl returns 0 there, and its last line, v[i] = (SEG && fl[c]) ? l[c] : base + l[c], may
drop `base` or ignore `fl[c]` without changing a bit they see.  Here the grid is never capped (CDH_COX_GRID is not set) and the
shapes are tests/_cox_runs_cases.py's: R6 (6 runs: past one lane), R301 (301 runs: past one wave, a partial last chunk) and
R1024 (1536 tiles in 1024 runs of one and two tiles: all four waves, carries from tile to tile inside a run, runs that lie
wholly inside one stratum, 1024 records into k_gram_reduce).  Every case asserts its shape on the CPU before a handle exists;
tests/test_cox_wide_host.py runs those asserts without a GPU.

Leg A, exact sums (strata and interval chains; tests/_cox_runs_cases.py's docstring has the construction).  Empty iterate, no
offset, weights np.ones(n) (the weighted instantiations run): every scanned sum is a small integer or ONE term among zeros,
so w, z, r and the counts out[2], out[3], out[4] are compared with == against closed forms; a wrong head flag, offset or carry
makes some S another integer.  out[1] keeps (n + 64) U sum w; out[0] = sum of log S over the events keeps the nll rule of
tests/test_gpu_cox_strata.py (the device's log is not the host's).  The leg supposes that the device's exp(0.0) is exactly 1;
a stratum of 2 rows says so first (w == 1/4), and LAB_NOTES.md "Cox lasso: the scan over the runs" records that it held.

Leg B, random data (all three chains): times rounded to a decimal so that tie groups straddle run edges, an offset, eta from a
two-coefficient iterate, and with strata 1000 to 2000 of them at R1024, sizes 2^k for k = 0 .. 13 drawn at random, weights
uniform in [0.25, 4].  The reference is the wide twin (tests/_cox_wide_numpy.py: longdouble cumulative sums per stratum,
rounded once; pinned to the fsum definitions in tests/test_cox_wide_host.py): the fsum definitions are quadratic, and the
double cumulative sums err by as much as the device may.  Its own error is at most about 3 n 2^-64 per sum, 2^-9 of the
(n + 10) U the device is allowed, so the bounds and the checking code are the three modules' own (_check_rows of each, with the
case's n), unwidened, and so is their rule that at least half of the training rows are unclamped.  One fold case per chain at
R1024 (fold 1 of 3, and a whole run's worth of consecutive sorted positions beside it: a stretch of e = 0 longer than a run) and
one repeat per chain (two handles, read-only and applied: the same bits).  Every case prints its worst multiples; LAB_NOTES.md
holds the ones seen on an MI355X."""
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_runs_cases as RC
import _cox_strata_numpy as CS
import _cox_wide_numpy as CW
from test_gpu_cox import _check_rows as _check_plain, _step
from test_gpu_cox_interval import _check_rows as _check_interval
from test_gpu_cox_strata import _check_rows as _check_strata

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
WMIN, EMAX = RC.WMIN, RC.EMAX
NAMES = list(RC.SHAPES)
CHAINS = ("plain", "strata", "interval")


def _y(start, t, status):
    return np.c_[t, status] if start is None else np.c_[start, t, status]


# ---- leg A: exact sums -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("chain", CHAINS[1:])
def test_exact_sums_at_every_run_offset(monkeypatch, name, chain):
    monkeypatch.delenv("CDH_COX_GRID", raising=False)
    c = RC.exact_case(name, chain == "interval")                 # (asserts the shape and the arrangement)
    n = RC.SHAPES[name]
    X = np.asfortranarray((np.arange(n) % 7 - 3.0).reshape(n, 1))
    f = cd.CDCoxLoss(_y(c["start"], c["time"], c["status"]), X, None, strata=c["g"], weights=np.ones(n))
    np.testing.assert_array_equal(f.weights, np.ones(n))
    cd.initialize_(f, cd.SparseIterate(1))
    np.testing.assert_array_equal(f.y - f.r, np.zeros(n))       # eta = 0 on every row
    ro = _step(f, -1, 0, WMIN, EMAX)
    out = _step(f, -1, 1, WMIN, EMAX)
    assert np.array_equal(ro, out)
    w, z, r = f.w, f.y, f.r
    f.close()
    two = (c["m"] == 2.0) & ~c["late_row"] & (c["w"] == 0.25)
    assert two.any()
    assert np.all(w[two] == 0.25), "exp(0.0) is not 1 on the device: w of a stratum of two rows is %r" % w[two][:4]
    bad = np.nonzero((w != c["w"]) | (r != c["r"]) | (z != c["r"]))[0]
    print(f"cox runs exact {chain} {name}: {len(c['sizes'])} strata, {int(c['late_strata'].sum())} late; rows off {len(bad)}; "
          f"clamped {int(out[2])} capped {int(out[3])} events {int(out[4])}; sum_w error / bound "
          f"{abs(out[1] - math.fsum(c['w'])) / ((n + 64) * U * math.fsum(c['w'])):.3f}")
    np.testing.assert_array_equal(w, c["w"])
    np.testing.assert_array_equal(r, c["r"])
    np.testing.assert_array_equal(z, c["r"])
    assert out[2] == c["out2"] and out[3] == 0.0 and out[4] == c["out4"]
    s_w = math.fsum(c["w"])
    assert abs(out[1] - s_w) <= (n + 64) * U * s_w
    # the nll by the rule of tests/test_gpu_cox_strata.py: the terms are log S, one per event, dv = 1
    logS = np.log(c["S_event"])
    err = abs(out[0] - math.fsum(logS))
    plain = (n + 65) * U * math.fsum(np.abs(logS))
    floor = math.fsum((n + 10) * U + 2 * U * np.abs(logS))
    assert err <= (plain + floor if plain < floor else plain), (err, plain, floor)


# ---- leg B: random rows against the wide twin ------------------------------------------------------------------------------------
def _handle(c):
    return cd.CDCoxLoss(_y(c["start"], c["time"], c["status"]), c["X"], c["off"], strata=c["g"], weights=c["v"])


def _iterate():
    x = cd.SparseIterate(2)
    x[1], x[2] = 0.8, -0.6
    return x


def _check(chain, tag, c, f, w, z, r, out, eta_lin, train):
    """The chain's own _check_rows against the wide twin at the eta the handle held; at least half of the training rows
    unclamped in every chain."""
    n = len(eta_lin)
    vn = f.weights if chain != "plain" else None
    q = CW.rows(eta_lin, c["off"], c["time"], c["status"], WMIN, EMAX, train, c["g"], vn, c["start"])
    tr = np.ones(n, dtype=bool) if train is None else train
    unc = tr & ~q["clamped"]
    assert unc.sum() >= tr.sum() / 2
    # the raw errors, which the modules' prints round away at these n: in units of U times the scale of each bound
    sc = tr & (q["delta"] + q["eA"] > 0.0)
    dw = (np.abs(w - q["w"])[unc] / (U * q["eA"][unc])).max()
    dr = (np.abs(r - q["r"])[sc] * q["w"][sc] / (U * (q["delta"] + q["eA"])[sc])).max()
    dn = abs(out[0] - math.fsum(q["nll"][tr])) / (U * math.fsum(np.abs(q["nll"][tr])))
    ds = abs(out[1] - math.fsum(q["w"][tr])) / (U * math.fsum(q["w"][tr]))
    print(f"{tag}: errors in units of U: |dw| / evA {dw:.1f}  |dr| w / (dv + evA) {dr:.1f}  nll / sum|terms| {dn:.1f}  sum_w {ds:.1f}")
    if chain == "plain":
        _check_plain(tag, n, w, z, r, out, q, eta_lin, train, WMIN)
    elif chain == "strata":
        _check_strata(tag, n, w, z, r, out, q, eta_lin, train, WMIN, unit=False)
    else:
        _check_interval(tag, n, c["g"], w, z, r, out, q, q, eta_lin, train, WMIN, unit=False)      # (the sizes are the wide twin's too)
    return q


def _arranged(name, chain, c):
    order, first, last, sfirst, slast = CS.groups(c["time"], c["g"])
    RC.assert_random_arrangement(name, chain, first, sfirst, slast)
    return order


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("chain", CHAINS)
def test_random_rows_against_the_wide_twin(monkeypatch, chain, name):
    monkeypatch.delenv("CDH_COX_GRID", raising=False)
    c = RC.random_case(name, chain)
    _arranged(name, chain, c)
    f = _handle(c)
    cd.initialize_(f, _iterate())
    eta_lin = f.y - f.r                                          # what the kernels recover, from the same two stored vectors
    ro = _step(f, -1, 0, WMIN, EMAX)
    out = _step(f, -1, 1, WMIN, EMAX)
    assert np.array_equal(ro, out)
    w, z, r = f.w, f.y, f.r
    q = _check(chain, f"runs {chain} {name}", c, f, w, z, r, out, eta_lin, None)
    assert out[3] > 0 and np.max(np.abs(eta_lin)) > 1.0         # some rows cap
    f.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_fold_and_a_run_of_held_rows_leave_the_risk_sets(monkeypatch, chain):
    """R1024, fold 1 of 3 held out and with it every row at the sorted positions of one whole two-tile run and five more on
    either side: that run's record is all zeros, and the offsets scan carries its neighbours' sums across it.  Held rows get
    w = 0, r = 0 and z = eta exactly; the training rows meet the step's bounds against the wide twin on the training rows."""
    monkeypatch.delenv("CDH_COX_GRID", raising=False)
    name, k = "R1024", 1
    c = RC.random_case(name, chain)
    n = RC.SHAPES[name]
    order = _arranged(name, chain, c)
    a, b = RC.held_stretch(name)
    ids = np.random.default_rng(n).permutation(n) % 3
    ids[order[a:b]] = k
    train = ids != k
    edges = RC.run_edges(n)
    assert not train[order[edges[511]:edges[512]]].any() and b - a > edges[512] - edges[511]
    assert c["status"][train].any()
    f = _handle(c)
    f.set_folds(ids, 3)
    cd.initialize_(f, _iterate())
    eta_lin = f.y - f.r
    ro = _step(f, k, 0, WMIN, EMAX)
    out = _step(f, k, 1, WMIN, EMAX)
    assert np.array_equal(ro, out)
    w, z, r = f.w, f.y, f.r
    np.testing.assert_array_equal(w[~train], 0.0)
    np.testing.assert_array_equal(r[~train], 0.0)
    np.testing.assert_array_equal(z[~train], eta_lin[~train])
    _check(chain, f"runs fold {chain} {name}", c, f, w, z, r, out, eta_lin, train)
    f.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_repeatable_across_handles_at_the_full_grid(monkeypatch, chain):
    """R1024: two handles, each read-only and applied -- the same bits in the record and in w, z, r."""
    monkeypatch.delenv("CDH_COX_GRID", raising=False)
    c = RC.random_case("R1024", chain)
    got = []
    for _ in range(2):
        f = _handle(c)
        cd.initialize_(f, _iterate())
        ro = _step(f, -1, 0, WMIN, EMAX)
        out = _step(f, -1, 1, WMIN, EMAX)
        got.append((ro, out, f.w, f.y, f.r))
        f.close()
    assert np.array_equal(got[0][0], got[0][1])
    for u, v in zip(*got):
        np.testing.assert_array_equal(u, v)
