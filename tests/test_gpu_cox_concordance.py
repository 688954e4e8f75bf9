"""Harrell's concordance index on the device: cdh_glm_cox_concordance (csrc/cox_concordance.hip), held to the definition
(tests/_cox_concordance_numpy.py: `definition`, every pair looked at; its two halves are pinned in
tests/test_cox_concordance_host.py) at the eta the handle held.

Unit weights, and weights drawn from {0.5, 1.5} in equal numbers (they already sum to n, so the front end's normalisation leaves
their bits, and every product and sum is a multiple of 1/4 far below 2^53): the three numbers are compared with ==.

Weights uniform in [0.25, 4], against the definition in long double, U = 2^-53: each of the three numbers is within
    (2n + 64) U (concordant + discordant + tied).
The summation order built (cox_concordance.hip).  A row's three sums L <= E <= G (the weight of the smaller, the smaller-or-equal
and all eta in its range) are each ONE chain of additions of non-negative terms: first the fringes position by position -- a
range inside two neighbouring tiles is all fringe, at most min(n - 1, 2 T - 1) terms and nothing else; otherwise at most
2 (T - 1) -- then at most two run values per level from the tile's to the one below the top, 2 (top - 10) of them.  A run value is a prefix sum
formed along the merge tree, one rounded addition per level, so it carries at most top roundings.  First order in U, with
A = max(min(n - 1, 2 T - 1), 2 (T - 1) + 2 (top - 10) + top):  |dL| <= A U L, and the same for E and G.  tied = E - L and
above = G - E round once more and inherit both errors: |d tied| <= A U (E + L) + U tied.  The products v L, v tied, v above round
once; the sum over the rows is block_sum's tree over a tile (2 + 6 + 4 levels) and a chain over the tiles by 256 lanes plus the
same tree, at most 12 + ceil(tiles / 256) + 12 <= 25 roundings here.  Summed with the weights v, sum v (E + L) = 2 concordant +
tied <= 2 (concordant + discordant + tied), so each number is within (2 A + 28) U (concordant + discordant + tied).  At the
sizes of this file: n = 2: 30; n = 65: 156; n = T + 1 (two tiles: every range is all fringe): 2 T + 28 = 2076 <= 2114;
n = 2 T + 1 (top = 12): 2 (2046 + 4 + 12) + 28 = 4152 <= 4162; n = 5 T + 3 (top = 13): 2 (2046 + 6 + 13) + 28 = 4158 <= 10310.
So the issue's (2n + 64) holds for this order and is what the test asserts.  Every weighted case prints its worst measured
multiple of the bound, which must be <= 1; LAB_NOTES.md "Cox lasso: concordance index" holds the ones seen on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_concordance_numpy as CC
import _cox_numpy as CX
import _cox_plan as CP

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
T = CP.TILE
LD = np.longdouble

SIZES = (1, 2, 65, T + 1, 2 * T + 1, 5 * T + 3)
TIMES = ("none", "one", "straddle")
ETAS = ("distinct", "decimal", "equal")
STRATA = ("single", "lane", "noevent", "lastevent")
WEIGHTS = ("unit", "half", "uniform")
# twelve combinations a size: every (time, strata) pair and every (time, eta) pair; the row order and the weights cycle
COMBOS = [(TIMES[i % 3], ETAS[(i // 3 + i) % 3], STRATA[i % 4], bool((i // 4 + i) % 2), WEIGHTS[(i // 2 + i // 6) % 3]) for i in range(12)]
CASES = [(n,) + c for n in SIZES for c in COMBOS]
IDS = ["n%d-%s-%s-%s-%s-%s" % (n, t, e, s, "sorted" if p else "random", w) for n, t, e, s, p, w in CASES]


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(f, k=-1):
    out = np.full(4, np.nan)
    cd.check(f._L.cdh_glm_cox_concordance(f._h, int(k), out.ctypes.data_as(C.POINTER(C.c_double))), f._h)
    return out


def _data(n, tpat, epat, spat, presorted, wkind):
    """In sorted layout -- by (stratum, time) -- and then dealt to the rows: the design's one column IS eta_lin (beta = 1), the
    offset is 0 or 0.5, so eta has the ties the pattern asks for."""
    rng = np.random.default_rng(7000 + n + 17 * TIMES.index(tpat) + 5 * ETAS.index(epat) + STRATA.index(spat))
    g = np.zeros(n, dtype=np.int64)
    bounds = [0, n]
    if spat != "single" and n > 2:
        # "lane": the boundary inside four consecutive positions, a lane's in the Cox step's scans, whose orders this call reads;
        # these kernels deal a tile's positions to the lanes 256 apart and carry nothing from one position to the next.  The
        # others: three strata
        bounds = [0, 4 * (n // 8) + 2, n] if spat == "lane" else [0, n // 3, 2 * (n // 3), n]
        for i, (a, b) in enumerate(zip(bounds, bounds[1:])):
            g[a:b] = (0, 4, 9)[i] if len(bounds) == 4 else (0, 7)[i]
    if tpat == "none":
        cuts = set(range(n))
    elif tpat == "one":
        cuts = set()
    else:                                                        # groups of 1 .. 7, and one across every tile edge
        cuts = set(np.cumsum(rng.integers(1, 8, n)).tolist())
        for edge in range(T, n, T):
            cuts -= set(range(edge - 2, edge + 3))
    cuts = sorted((cuts | set(bounds)) & set(range(n)))
    gid = np.searchsorted(np.array(cuts), np.arange(n), side="right") - 1
    t = np.full(n, 2.5) if tpat == "one" else 1.0 + 0.5 * gid
    status = (rng.random(n) < 0.7).astype(np.float64)
    if spat == "noevent" and n > 2:
        status[g == 4] = 0.0
    if spat == "lastevent" and n > 2:
        status[gid == gid[-1]] = 1.0                             # a group of events only: the last position holds an event
    if not status.any():
        status[0] = 1.0
    eta_lin = dict(distinct=rng.normal(0.0, 1.0, n), decimal=np.round(rng.normal(0.0, 0.6, n), 1), equal=np.full(n, 0.3))[epat]
    off = np.zeros(n) if epat == "equal" else 0.5 * rng.integers(0, 2, n)
    if wkind == "unit":
        v = None
    elif wkind == "half":
        v = rng.permutation(np.r_[np.full(n // 2, 0.5), np.full(n // 2, 1.5), np.ones(n % 2)])
    else:
        v = rng.uniform(0.25, 4.0, n)
    if not presorted:
        perm = rng.permutation(n)
        g, t, status, eta_lin, off = g[perm], t[perm], status[perm], eta_lin[perm], off[perm]
        v = None if v is None else v[perm]
    if n >= 3:                                                   # two folds and a third of one row
        ids = rng.integers(0, 2, n).astype(np.int32)
        ids[:2] = (0, 1)
        ids[rng.integers(2, n)] = 2
    else:
        ids = np.arange(n, dtype=np.int32)
    return g if np.any(g != g[0]) else None, t, status, eta_lin, off, v, ids


def _want(wkind, t, status, eta, g, vn, subset):
    dt = LD if wkind == "uniform" else np.float64
    return CC.definition(t, status, eta, strata=g, weights=vn, subset=subset, dtype=dt)


@pytest.mark.parametrize("n,tpat,epat,spat,presorted,wkind", CASES, ids=IDS)
def test_counts_against_the_definition(n, tpat, epat, spat, presorted, wkind):
    g, t, status, eta_lin, off, v, ids = _data(n, tpat, epat, spat, presorted, wkind)
    f = cd.CDCoxLoss(np.c_[t, status], np.asfortranarray(eta_lin[:, None]), off, strata=g, weights=v)
    x = cd.SparseIterate(1)
    x[1] = 1.0
    cd.initialize_(f, x)
    eta = (f.y - f.r) + off
    np.testing.assert_array_equal(f.y - f.r, eta_lin)
    vn = None
    if v is not None:
        vn = f.weights
        if wkind == "half":
            np.testing.assert_array_equal(vn, v)                 # the stored weights are those bits
    K = int(ids.max()) + 1
    subsets = [(-1, None)]
    if n >= 2:
        count = f.set_folds(ids, K)
        assert n < 3 or count[2] == 1
        subsets += [(k, ids == k) for k in range(K)]
    worst = 0.0
    results = []
    for k, subset in subsets:
        got = _call(f, k)
        want = _want(wkind, t, status, eta, g, vn, subset)
        assert got[3] == 0.0
        if wkind == "uniform":
            tot = float(want[0] + want[1] + want[2])
            bound = (2 * n + 64) * U * tot
            err = max(abs(float(LD(got[i]) - want[i])) for i in range(3))
            if tot == 0.0:
                assert tuple(got[:3]) == (0.0, 0.0, 0.0)
            else:
                worst = max(worst, err / bound)
        else:
            assert tuple(got[:3]) == tuple(float(w) for w in want), (k, got, want)
        results.append(got)
        c = f.concordance(None if k < 0 else k)
        assert (c.concordant, c.discordant, c.tied, c.comparable) == (got[0], got[1], got[2], got[0] + got[1] + got[2])
        assert c.C == CC.cindex(*got[:3]) or (np.isnan(c.C) and c.comparable == 0)
    if wkind == "uniform":
        print(f"concordance {IDS[CASES.index((n, tpat, epat, spat, presorted, wkind))]}: worst multiple of (2n + 64) U total {worst:.3e}")
        assert worst <= 1.0
    if epat == "equal":
        assert results[0][0] == 0.0 and results[0][1] == 0.0 and (results[0][2] == 0.0 or f.concordance().C == 0.5)
    if n >= 65 and tpat != "one" or n >= 65 and spat == "single":
        assert results[0][:3].sum() > 0
    # the tie rule does not enter: the same bits on the handle set to Efron
    f.set_ties("efron")
    for (k, _), before in zip(subsets, results):
        np.testing.assert_array_equal(_call(f, k), before)
    assert cd.coxConcordance(f).C == f.concordance().C or np.isnan(f.concordance().C)
    f.close()


def _fitted(n=2 * T + 1, weights=True, seed=5):
    X, t, s, off = CX.make_data(n, 3, seed, decimals=1, censor=0.3, with_offset=True)
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, n) * 5 - 5
    v = rng.uniform(0.25, 4.0, n) if weights else None
    f = cd.CDCoxLoss(np.c_[t, s], X, off, strata=g, weights=v)
    x = cd.SparseIterate(3)
    x[1], x[3] = 0.7, -0.4
    cd.initialize_(f, x)
    f.irls_step(apply=True)
    return f, (X, t, s, off, g)


def _beta(f):
    b = np.full(f.p, np.nan)
    cd.check(f._L.cdh_get_beta(f._h, b.ctypes.data_as(C.POINTER(C.c_double))), f._h)
    return b


def test_the_call_is_read_only_and_repeatable():
    f, (X, t, s, off, g) = _fitted()
    n = f.n
    ids = (np.arange(n) % 3).astype(np.int32)
    f.set_folds(ids, 3)
    rec0 = f.irls_step(apply=False)
    y0, r0, w0, b0 = f.y, f.r, f.w, _beta(f)
    first = [_call(f, k) for k in (-1, 0, 1, 2)]
    second = [_call(f, k) for k in (-1, 0, 1, 2)]
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(f.y, y0)
    np.testing.assert_array_equal(f.r, r0)
    np.testing.assert_array_equal(f.w, w0)
    np.testing.assert_array_equal(_beta(f), b0)
    assert f.irls_step(apply=False) == rec0                      # the step's scratch serves the step as before
    np.testing.assert_array_equal(_call(f, -1), first[0])
    # the held-out rows of the folds are disjoint subsets: no fold's comparable pairs exceed the whole's
    assert all(a[:3].sum() < first[0][:3].sum() for a in first[1:])
    # new survival data on the same handle: the order is derived again
    t2 = np.round(t[::-1].copy() + 0.3, 1)
    cd.check(f._L.cdh_glm_set_survival_strata(f._h, _vp(t2), _vp(np.ascontiguousarray(s)), None, None, None), f._h)
    got = _call(f, -1)
    eta = f.y - f.r
    assert tuple(got[:3]) == CC.definition(t2, s, eta) and got[:3].sum() > 0
    f.close()


def test_refusals():
    f, (X, t, s, off, g) = _fitted(65, weights=False)
    L, h, n = f._L, f._h, f.n
    err = lambda: L.cdh_last_error(h).decode()
    out = np.full(4, -3.0)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    y0, r0 = f.y, f.r
    assert L.cdh_glm_cox_concordance(h, -2, po) == BAD and "k must be" in err()
    assert L.cdh_glm_cox_concordance(h, 0, po) == BAD and "cdh_set_folds" in err()
    f.set_folds((np.arange(n) % 3).astype(np.int32), 3)
    assert L.cdh_glm_cox_concordance(h, 3, po) == BAD and "below the K" in err()
    assert L.cdh_glm_cox_concordance(h, 2, None) == BAD and "out4 is NULL" in err()
    f.set_host_exchange(lambda buf: None, 0, 1)                  # an exchange installed makes the handle a row shard
    assert L.cdh_glm_cox_concordance(h, -1, po) == BAD and "row-sharded" in err()
    f.set_host_exchange(None, 0, 1)
    assert np.all(out == -3.0)
    assert L.cdh_glm_cox_concordance(h, 2, po) == OK and out[3] == 0.0
    np.testing.assert_array_equal(f.y, y0)
    np.testing.assert_array_equal(f.r, r0)
    f.close()
    # start-stop times
    y3 = np.c_[t - 0.5 - (np.arange(n) % 2), t, s]
    for first in (X, cd.CDCoxLoss(y3, X, off)):                  # the front end refuses before any upload or solve
        with pytest.raises(cd.ArgumentError, match="not offered yet"):
            cd.cvCoxLassoPath(first, y3 if first is X else None, [0.1], K=3, measure="C")
    iv = cd.CDCoxLoss(y3, X, off)
    assert iv._L.cdh_glm_cox_concordance(iv._h, -1, po) == BAD
    assert "concordance with start-stop times is not offered yet" in iv._L.cdh_last_error(iv._h).decode()
    with pytest.raises(cd.ArgumentError, match="not offered yet"):
        iv.concordance()
    iv.close()
    # a binomial handle, and a handle before any observations
    b = cd.CDLogisticLoss((s > 0).astype(np.float64), X)
    assert b._L.cdh_glm_cox_concordance(b._h, -1, po) == BAD and "no survival data" in b._L.cdh_last_error(b._h).decode()
    b.close()
    w = cd.CDWeightedLSLoss(np.zeros(n), X, np.ones(n))
    assert w._L.cdh_glm_cox_concordance(w._h, -1, po) == BAD and "no survival data" in w._L.cdh_last_error(w._h).decode()
    w.close()


def test_a_nan_is_counted_and_the_front_end_raises():
    f, (X, t, s, off, g) = _fitted(T + 1, weights=False)
    n = f.n
    ids = (np.arange(n) % 3).astype(np.int32)
    f.set_folds(ids, 3)
    y = f.y
    y[4] = np.nan                                                # row 4 lies in fold 1
    cd.check(f._L.cdh_set_y(f._h, _vp(y)), f._h)
    assert _call(f, -1)[3] == 1.0 and _call(f, 1)[3] == 1.0
    for k in (0, 2):
        got = _call(f, k)
        eta = (f.y - f.r) + off
        assert got[3] == 0.0 and tuple(got[:3]) == CC.definition(t, s, eta, strata=g, subset=ids == k)
    with pytest.raises(cd.ArgumentError, match="NaN in 1 of the rows"):
        f.concordance()
    with pytest.raises(cd.ArgumentError, match="NaN"):
        cd.coxConcordance(f, fold=1)
    assert f.concordance(fold=0).comparable > 0
    f.close()


def test_cv_path_by_the_concordance_index():
    """n = 300, p = 8, 3 folds, 4 lambda, strata and an offset: fold_concordance is the definition on the held-out rows at the eta
    downloaded from a handle that holds the fold path's beta; the selection maximises; the deviance run is bit for bit the same."""
    n, K, P = 300, 3, 8
    X, t, s, off = CX.make_data(n, P, 11, decimals=1, censor=0.3, with_offset=True)
    rng = np.random.default_rng(12)
    g = rng.integers(0, 2, n) * 3
    y = np.c_[t, s]
    ids = (rng.permutation(n) % K).astype(np.int32)
    f0 = cd.CDCoxLoss(y, X, off, strata=g)
    lmax = cd.coxLambdaMax(f0)
    lams = np.geomspace(0.7, 0.1, 4) * lmax
    kw = dict(K=K, folds=ids, offset=off, strata=g, keep_fold_paths=True, options=cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False),
              irls=cd.IRLSOptions(maxIter=100, optTol=1e-10))
    res = cd.cvCoxLassoPath(X, y, lams, measure="C", **kw)
    assert isinstance(res, cd.CVCoxConcordancePathResult) and res.measure == "C" and res.fold_concordance.shape == (K, 4)
    for k in range(K):
        for j in range(4):
            cd.initialize_(f0, res.fold_paths[k].betapath[j])
            eta = (f0.y - f0.r) + off
            want = CC.definition(t, s, eta, strata=g, subset=ids == k)
            assert res.fold_concordance[k, j] == CC.cindex(*want), (k, j)
    assert np.all((res.fold_concordance > 0.5) & (res.fold_concordance < 1.0))         # the model does rank the held-out rows
    f0.close()
    wt = np.bincount(ids, minlength=K) / n
    cvm = wt @ res.fold_concordance
    cvsd = np.sqrt(wt @ (res.fold_concordance - cvm) ** 2 / (K - 1))
    np.testing.assert_array_equal(res.cvm, cvm)
    np.testing.assert_array_equal(res.cvsd, cvsd)
    imax = int(np.argmax(cvm))
    assert res.index_min == imax and res.lambda_min == lams[imax]
    ok = np.nonzero(cvm >= cvm[imax] - cvsd[imax])[0]
    assert res.index_1se == int(ok[np.argmax(lams[ok])]) and res.lambda_1se == lams[res.index_1se] and res.index_1se <= imax
    dev = cd.cvCoxLassoPath(X, y, lams, measure="deviance", **kw)
    assert type(dev) is cd.CVCoxLassoPathResult and dev.measure == "deviance"
    np.testing.assert_array_equal(dev.fold_deviance, res.fold_deviance)
    np.testing.assert_array_equal(dev.train_deviance, res.train_deviance)
    np.testing.assert_array_equal(dev.rounds, res.rounds)
    np.testing.assert_array_equal(dev.fold_events, res.fold_events)
    for a, b in zip(dev.path.betapath, res.path.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())
    # a fold whose held-out rows hold no comparable pair is refused, by its number
    lone = np.where(np.arange(n) == int(np.nonzero(s == 1.0)[0][0]), 2, np.arange(n) % 2).astype(np.int32)
    with pytest.raises(cd.ArgumentError, match="fold 2 holds no comparable pair"):
        cd.cvCoxLassoPath(X, y, lams[:1], measure="C", **dict(kw, folds=lone))
