"""cdh_glm_cox_score on the device (csrc/cox_score.hip, over the scratch of the handle's own read-only step): Schoenfeld residuals,
score residuals and the information matrix, held to the numpy twin's scan half in long double (tests/_cox_score_numpy.py; its
halves are pinned in tests/test_cox_score_host.py) at the eta the handle held, for the plain chain and for strata with weights,
rows in random order and pre-sorted, at the sizes and tie and strata patterns of tests/test_gpu_cox_post.py, with p = 70 columns.

The bounds, derived from the two the project already holds (tests/test_gpu_cox_strata.py): |dS| <= (n + 10) U S and
|dA| <= (2n + 18) U A.  U = 2^-53, first order in U, the twin's long-double values taken as exact (their own error is 2^-11 of
these bounds); xt = x - centre is the same double on both sides (the twin is given the centres the device used).  Everything is
inside the row's own stratum.
    N      a suffix scan of at most n signed terms ev xt.  A term carries ev's error (the device's exp against numpy's, the
           product v e: inside the S bound's constant) and one more product, so as for S with one more rounding, but relative to the
           scan of the ABSOLUTE values, Nabs = sum ev |xt|:          |dN| <= (n + 11) U Nabs.
    xbar   = N / S:  |dN| / S + |xbar| |dS| / S + U |xbar|, and |xbar| <= Xabs = Nabs / S:
                                                                      |dxbar| <= (2n + 22) U Xabs.
    sch    = xt - xbar, one more rounding:                            |dsch| <= (2n + 22) U Xabs + U |sch|.
    h      = dv / S: dv exact, S's bound, one division: (n + 11) U h.
    Q      a prefix scan of at most n terms h xbar.  A term: h (n + 11) U |xbar| + h (2n + 22) U Xabs + U h |xbar|
           <= (3n + 34) U h Xabs; the scan adds n U of the absolute scan Qabs = sum h Xabs:
                                                                      |dQ| <= (4n + 34) U Qabs.
    L      = sch - e (xt A - Q).  xt A: A's bound and a product, (2n + 19) U |xt| A; less Q: its bound and U (|xt| A + Qabs);
           times e: exp against numpy's and a product, 2 U more; all below (4n + 40) U e (|xt| A + Qabs); the last subtraction
           U |L|:                                                     |dL| <= |dsch| + (4n + 40) U e (|xt| A + Qabs) + U |L|.
    I      first sum, at most n terms ev A xt_c xt_d: ev 2 U, A (2n + 18) U, three products, the additions n U:
           (3n + 23) U I1abs, I1abs = sum ev A |xt_c| |xt_d|.  Second sum, terms dv xbar_c xbar_d: two xbar (2n + 22) U each relative
           to Xabs, two products, the additions n U: (5n + 46) U I2abs, I2abs = sum dv Xabs_c Xabs_d.  One subtraction.  Relative
           to the SUM of the two absolute sums, not to I:             |dI| <= (5n + 47) U (I1abs + I2abs).
Every case prints the worst measured multiple of each bound, which must be <= 1; LAB_NOTES.md "Cox lasso: score residuals and the
information matrix" holds the ones seen on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_plan as CP
import _cox_score_numpy as CSN
import _cox_strata_numpy as CS
import test_gpu_cox_post as PG
from test_gpu_cox import _step, _vp

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
T = CP.TILE
FULL = CP.MAX_GRID
EMAX = PG.EMAX
LD = np.longdouble
P = 70
PAIR = 4                                                          # kCoxScorePair

CHAINS = ("plain", "strata")
CASES = [(n, cap, pat, chain, presorted) for n, cap in PG.SIZES for chain in CHAINS
         for pat in (PG.TIES if chain == "plain" else PG.TIES + PG.STRATA) for presorted in (False, True)]
IDS = ["n%d-cap%d-%s-%s-%s" % (n, cap, pat, chain, "sorted-unit" if s else "random-weighted") for n, cap, pat, chain, s in CASES]

# the column lists: non-contiguous and unsorted; the list of 64 holds column 17 twice (positions 3 and 40)
_rng = np.random.default_rng(99)
LIST64 = _rng.permutation(np.arange(1, P + 1))[:64].astype(np.int64)
LIST64[3] = 17
LIST64[40] = 17
LISTS = {1: np.array([23], dtype=np.int64), PAIR - 1: np.array([70, 2, 41], dtype=np.int64),
         PAIR + 1: np.array([9, 66, 1, 30, 12], dtype=np.int64), 64: LIST64}

_DATA = {}


def _data(n, cap, pattern, chain, presorted, integer=False):
    """The survival data of tests/test_gpu_cox_post.py's case, a design of P standard-normal columns (integer: entries in
    -3 .. 3) and an iterate on six of them.  Computed once per case and left unchanged."""
    key = (n, cap, pattern, chain, presorted, integer)
    if key not in _DATA:
        _, _, t, status, off, g, v, _ = PG._data(n, cap, pattern, chain, presorted)
        rng = np.random.default_rng(7000 + n + (1 if integer else 0))
        X = np.asfortranarray(rng.integers(-3, 4, (n, P)).astype(np.float64) if integer else rng.standard_normal((n, P)))
        X.setflags(write=False)
        x = cd.SparseIterate(P)
        for j, b in zip((2, 9, 17, 23, 41, 66), (0.8, -0.6, 0.4, -0.3, 0.5, 0.2)):
            x[j] = b
        _DATA[key] = (X, t, status, off, g, v, x)
    return _DATA[key]


def _loss(monkeypatch, X, t, status, off, g, v, cap=FULL):
    if cap != FULL:
        monkeypatch.setenv("CDH_COX_GRID", str(cap))            # read when the handle is made
    return cd.CDCoxLoss(np.c_[t, status], X, off, strata=g, weights=v)


def _score(f, cols, centre=None, want=(True, True, True), eta_max=EMAX):
    """-> (status, sch, L, I, the centres used); an output not wanted is None and its pointer NULL."""
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    m = len(cols)
    sch = np.full((f.n, m), np.nan, order="F") if want[0] else None
    L = np.full((f.n, m), np.nan, order="F") if want[1] else None
    I = np.full((m, m), np.nan) if want[2] else None
    used = np.full(m, np.nan)
    st = f._L.cdh_glm_cox_score(f._h, float(eta_max), m, _vp(cols), _vp(centre), _vp(used), _vp(sch), _vp(L), _vp(I))
    return st, sch, L, I, used


def _bounds(n, q):
    f64 = lambda a: np.abs(np.asarray(a, dtype=np.float64))
    Xabs, Qabs = f64(q["Xabs"]), f64(q["Qabs"])
    e, A = f64(q["e"])[:, None], f64(q["A"])[:, None]
    bs = np.where(q["counts"][:, None], (2 * n + 22) * U * Xabs + U * f64(q["sch"]), 0.0)
    bL = bs + (4 * n + 40) * U * e * (f64(q["xt"]) * A + Qabs) + U * f64(q["score"])
    bI = (5 * n + 47) * U * (f64(q["I1abs"]) + f64(q["I2abs"]))
    return bs, bL, bI


_worst, _err = PG._worst, PG._err


def _twin(f, X, cols, t, status, off, g, used, eta_lin):
    return CSN.scan(X[:, cols - 1], eta_lin, off, t, status, EMAX, strata=g, weights=f.weights, centre=used)


# ---- against the twin, case by case ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,pattern,chain,presorted", CASES, ids=IDS)
def test_against_the_twin(monkeypatch, n, cap, pattern, chain, presorted):
    X, t, status, off, g, v, x = _data(n, cap, pattern, chain, presorted)
    tag = IDS[CASES.index((n, cap, pattern, chain, presorted))]
    f = _loss(monkeypatch, X, t, status, off, g, v, cap)
    cd.initialize_(f, x)
    y0, r0 = f.y, f.r
    eta_lin = y0 - r0
    rec0 = _step(f, -1, 0)
    cols = LISTS[64]
    st, sch, L, I, used = _score(f, cols)
    assert st == OK, f._L.cdh_last_error(f._h)
    # the centres: the columns' means, in the kernel's own order: n additions and a division
    mean = X[:, cols - 1].astype(LD).mean(axis=0)
    assert np.all(_err(used, mean) <= (n + 2) * U * np.abs(X[:, cols - 1]).mean(axis=0))
    q = _twin(f, X, cols, t, status, off, g, used, eta_lin)
    bs, bL, bI = _bounds(n, q)
    m = {"sch": _worst(_err(sch, q["sch"]), bs), "L": _worst(_err(L, q["score"]), bL), "I": _worst(_err(I, q["info"]), bI)}
    print(f"cox score {tag}: {int(q['counts'].sum())} events that count; worst multiples of the bounds: "
          + " ".join(f"{k} {val:.3f}" for k, val in m.items()))
    assert all(val <= 1.0 for val in m.values()), m
    assert np.all(sch[~q["counts"]] == 0.0)                      # exactly zero off the events
    assert np.array_equal(I, I.T)                                # symmetric by construction
    # purity: bit-identical on a second call; y, w, r and beta are what they were; the step's record does not move
    st2, sch2, L2, I2, used2 = _score(f, cols)
    assert st2 == OK
    for a, b in ((sch, sch2), (L, L2), (I, I2), (used, used2)):
        np.testing.assert_array_equal(a, b)
    for a, b in ((f.y, y0), (f.r, r0)):
        np.testing.assert_array_equal(a, b)
    beta = np.zeros(f.p)
    cd.check(f._L.cdh_get_beta(f._h, _vp(beta)), f._h)
    np.testing.assert_array_equal(beta, x.dense())
    assert np.array_equal(_step(f, -1, 0), rec0)
    # the duplicate columns, and one output alone with the others NULL: the same bits
    np.testing.assert_array_equal(sch[:, 3], sch[:, 40])
    np.testing.assert_array_equal(L[:, 3], L[:, 40])
    np.testing.assert_array_equal(I[3], I[40])
    _, _, only, _, _ = _score(f, cols, want=(False, True, False))
    np.testing.assert_array_equal(only, L)
    f.close()


# ---- the exact case ------------------------------------------------------------------------------------------------------------
EXACT = [(c, i) for c, i in zip(CASES, IDS) if c[4] and c[2] in ("straddle", "strata", "laststratum")]


@pytest.mark.parametrize("n,cap,pattern,chain,presorted", [c for c, _ in EXACT], ids=[i for _, i in EXACT])
def test_exact_case(monkeypatch, n, cap, pattern, chain, presorted):
    """Integer X in -3 .. 3, beta = 0, no offset, unit weights, centres 0: every ev is 1, S and N are exact integers in any order
    of summation, xbar = N / S is one rounding and sch is numpy's x - N / S with ==: an indexing error at a tile, run or stratum
    edge cannot hide in a bound.  L and I are NOT compared with ==: A is a sum of the quotients 1 / S, no integer, so ev A, the
    factor of I's first sum, is rounded and its sum depends on the order; they are held to the docstring's bounds, and an index
    that is wrong at an edge moves them by whole entries of X, orders of magnitude beyond those."""
    X, t, status, _, g, v, _ = _data(n, cap, pattern, chain, presorted, integer=True)
    assert v is None
    f = _loss(monkeypatch, X, t, status, None, g, None, cap)
    cd.initialize_(f, cd.SparseIterate(P))
    cols = LISTS[64]
    st, sch, L, I, used = _score(f, cols, centre=np.zeros(64))
    assert st == OK, f._L.cdh_last_error(f._h)
    assert np.all(used == 0.0)
    order, first, last, sfirst, slast = CS.groups(t, g)
    xs = X[:, cols - 1][order]
    ones = np.ones(n)
    S = CSN._seg_cumsum(ones, sfirst, slast, reverse=True)[first]
    want = np.zeros((n, 64))
    for c in range(64):
        N = CSN._seg_cumsum(xs[:, c].copy(), sfirst, slast, reverse=True)[first]
        want[order, c] = np.where(status[order] != 0, xs[:, c] - N / S, 0.0)
    np.testing.assert_array_equal(sch, want)
    q = CSN.scan(X[:, cols - 1], np.zeros(n), None, t, status, EMAX, strata=g, centre=np.zeros(64))
    bs, bL, bI = _bounds(n, q)
    assert _worst(_err(L, q["score"]), bL) <= 1.0 and _worst(_err(I, q["info"]), bI) <= 1.0
    f.close()


# ---- determinism and batching ----------------------------------------------------------------------------------------------------
BATCH = [(c, i) for c, i in zip(CASES, IDS) if c[:2] in ((65, FULL), (5 * T + 3, 2)) and c[2] in ("straddle", "noevent") and not c[4]]


@pytest.mark.parametrize("n,cap,pattern,chain,presorted", [c for c, _ in BATCH], ids=[i for _, i in BATCH])
def test_determinism_and_batching(monkeypatch, n, cap, pattern, chain, presorted):
    X, t, status, off, g, v, x = _data(n, cap, pattern, chain, presorted)
    f = _loss(monkeypatch, X, t, status, off, g, v, cap)
    cd.initialize_(f, x)
    big = LISTS[64]
    _, sch, L, I, used = _score(f, big)
    # every column of the m = 64 call == its own m = 1 call
    for c, col in enumerate(big):
        st, s1, l1, i1, u1 = _score(f, [col])
        assert st == OK
        np.testing.assert_array_equal(s1[:, 0], sch[:, c])
        np.testing.assert_array_equal(l1[:, 0], L[:, c])
        assert i1[0, 0] == I[c, c] and u1[0] == used[c]
    # the shorter lists (the pair tile's width less and plus one), and a permuted list: the permuted answers
    for m in (PAIR - 1, PAIR + 1):
        cols = LISTS[m]
        at = [int(np.nonzero(big == c)[0][0]) if c in big else None for c in cols]
        st, s2, l2, i2, _ = _score(f, cols)
        assert st == OK and np.array_equal(i2, i2.T)
        st, s3, l3, i3, _ = _score(f, cols[::-1].copy())
        np.testing.assert_array_equal(s3, s2[:, ::-1])
        np.testing.assert_array_equal(l3, l2[:, ::-1])
        np.testing.assert_array_equal(i3, i2[::-1, ::-1])
        for k, a in enumerate(at):
            if a is not None:
                np.testing.assert_array_equal(s2[:, k], sch[:, a])
                np.testing.assert_array_equal(l2[:, k], L[:, a])
                for k2, a2 in enumerate(at):
                    if a2 is not None:
                        assert i2[k, k2] == I[a, a2]
    perm = np.random.default_rng(5).permutation(64)
    _, sp, lp, ip, _ = _score(f, big[perm])
    np.testing.assert_array_equal(sp, sch[:, perm])
    np.testing.assert_array_equal(lp, L[:, perm])
    np.testing.assert_array_equal(ip, I[np.ix_(perm, perm)])
    f.close()


# ---- the handle ----------------------------------------------------------------------------------------------------------------
def test_the_handle_regrowth_ties_and_refusals(monkeypatch):
    n, cap, pattern = 2 * T + 1, FULL, "straddle"
    X, t, status, off, g, v, x = _data(n, cap, pattern, "strata", False)
    f = _loss(monkeypatch, X, t, status, off, g, v)
    Lb, h = f._L, f._h
    err = lambda: Lb.cdh_last_error(h).decode()
    cd.initialize_(f, x)
    _step(f, -1, 1)                                              # an applied step: the handle holds working weights from here on
    y0, r0, w0 = f.y, f.r, f.w
    # m = 1, then 64, then 1: the scratch regrows and the small call runs in the large group
    st, s1, l1, i1, u1 = _score(f, LISTS[1])
    assert st == OK
    st, s64, l64, i64, u64 = _score(f, LISTS[64])
    assert st == OK
    st, s1b, l1b, i1b, u1b = _score(f, LISTS[1])
    assert st == OK
    for a, b in ((s1, s1b), (l1, l1b), (i1, i1b), (u1, u1b)):
        np.testing.assert_array_equal(a, b)
    q = _twin(f, X, LISTS[64], t, status, off, g, u64, y0 - r0)
    bs, bL, bI = _bounds(n, q)
    assert _worst(_err(s64, q["sch"]), bs) <= 1.0 and _worst(_err(l64, q["score"]), bL) <= 1.0 and _worst(_err(i64, q["info"]), bI) <= 1.0
    # given centres: used as given and returned
    given = np.linspace(-1.0, 1.0, 64)
    st, sg, lg, ig, ug = _score(f, LISTS[64], centre=given)
    assert st == OK and np.array_equal(ug, given)
    qg = _twin(f, X, LISTS[64], t, status, off, g, given, y0 - r0)
    bs, bL, bI = _bounds(n, qg)
    assert _worst(_err(sg, qg["sch"]), bs) <= 1.0 and _worst(_err(lg, qg["score"]), bL) <= 1.0 and _worst(_err(ig, qg["info"]), bI) <= 1.0
    # Efron: refused with its message; back at Breslow: served, equal to what it was
    f.set_ties("efron")
    st, *_ = _score(f, LISTS[1])
    assert st == BAD and "cdh_glm_cox_score is not offered with Efron ties yet" in err()
    f.set_ties("breslow")
    st, s1c, l1c, i1c, _ = _score(f, LISTS[1])
    assert st == OK
    for a, b in ((s1, s1c), (l1, l1c), (i1, i1c)):
        np.testing.assert_array_equal(a, b)
    # every CDH_BAD_ARG of the header
    one = LISTS[1]
    for bad in (0.0, -1.0, 700.5, float("nan"), float("inf")):
        assert _score(f, one, eta_max=bad)[0] == BAD and "eta_max" in err()
    out = np.zeros((n, 65), order="F")
    idx65 = np.arange(1, 66, dtype=np.int64)
    assert Lb.cdh_glm_cox_score(h, EMAX, 0, _vp(idx65), None, None, _vp(out), None, None) == BAD and "1 <= m <= 64" in err()
    assert Lb.cdh_glm_cox_score(h, EMAX, 65, _vp(idx65), None, None, _vp(out), None, None) == BAD and "1 <= m <= 64" in err()
    assert Lb.cdh_glm_cox_score(h, EMAX, 1, None, None, None, _vp(out), None, None) == BAD and "idx1 is NULL" in err()
    for badcol in (0, P + 1, -3):
        assert _score(f, [badcol])[0] == BAD and "out of range" in err()
    assert _score(f, one, want=(False, False, False))[0] == BAD and "all NULL" in err()
    for badc in (float("nan"), float("inf")):
        assert _score(f, one, centre=np.array([badc]))[0] == BAD and "host_centre[0]" in err() and "not finite" in err()
    for a, b in ((f.y, y0), (f.r, r0), (f.w, w0)):
        np.testing.assert_array_equal(a, b)
    f.close()
    # start-stop times; a handle without survival data
    Xi, start, ti, si, oi, gi, vi, _ = PG._data(65, FULL, "straddle", "interval", False)
    fi = cd.CDCoxLoss(np.c_[start, ti, si], Xi, oi, strata=gi, weights=vi)
    cd.initialize_(fi, cd.SparseIterate(3))
    assert _score(fi, [1])[0] == BAD and "cdh_glm_cox_score is not offered with start-stop times yet" in fi._L.cdh_last_error(fi._h).decode()
    fi.close()
    b = cd.CDLogisticLoss((si > 0).astype(np.float64), Xi)
    assert _score(b, [1])[0] == BAD and "no survival data" in b._L.cdh_last_error(b._h).decode()
    b.close()
    # a handle that never asks allocates nothing more: a plain handle turned to Efron and back is served as well
    Xp, tp, sp_, op, gp, vp_, xp = _data(65, FULL, "straddle", "plain", False)
    fp = _loss(monkeypatch, Xp, tp, sp_, op, gp, vp_)
    cd.initialize_(fp, xp)
    st, a0, b0, c0, _ = _score(fp, LISTS[PAIR + 1])
    fp.set_ties("efron")
    fp.set_ties("breslow")
    st2, a1, b1, c1, _ = _score(fp, LISTS[PAIR + 1])
    assert st == OK and st2 == OK
    for a, b_ in ((a0, a1), (b0, b1), (c0, c1)):
        np.testing.assert_array_equal(a, b_)                     # the segmented chain over the defaults gives the plain chain's bits
    fp.close()


# ---- the gradient identity on the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", [(2 * T + 1, FULL), (5 * T + 3, 2)])
def test_column_sums_are_the_gradient_the_handle_holds(monkeypatch, n, cap):
    """sum_i v_i L_ic = Xt_c'(dv - ev A) = X_c' d, because sum d = 0 inside every stratum.  The handle gives X_c'(w r) after an
    applied step (cdh_xt_r_cols, no n-sized download), where r = d / w is the step's own residual at the eta the score call saw:
    the score call comes first, the step changes y and r.  The tolerance: the rows' L bounds; the step's |dd| <= (2n + 68) U
    (dv + ev A) (tests/test_gpu_cox_post.py's bM times v), the rounding of (d / w) w, 2 U |d|, and of a dot product of n terms,
    n U |x| |d|; the column sums here are taken in long double."""
    X, t, status, off, g, v, x = _data(n, cap, "noevent", "strata", False)
    f = _loss(monkeypatch, X, t, status, off, g, v, cap)
    cd.initialize_(f, x)
    eta_lin = f.y - f.r
    cols = LISTS[64]
    st, _, L, _, used = _score(f, cols, want=(False, True, False))
    assert st == OK
    _step(f, -1, 1)
    got = np.zeros(64)
    cd.check(f._L.cdh_xt_r_cols(f._h, 64, _vp(cols), _vp(got)), f._h)
    vn = f.weights
    q = _twin(f, X, cols, t, status, off, g, used, eta_lin)
    _, bL, _ = _bounds(n, q)
    lhs = (vn[:, None].astype(LD) * L.astype(LD)).sum(axis=0)
    d = (q["dv"] - q["ev"] * q["A"]).astype(np.float64)
    size = (q["dv"] + q["ev"] * q["A"]).astype(np.float64)
    Xa = np.abs(X[:, cols - 1])
    tol = vn @ bL + Xa.T @ ((2 * n + 68) * U * size + (n + 2) * U * np.abs(d))
    worst = _worst(np.abs((lhs - got).astype(np.float64)), tol)
    print(f"cox score n={n} cap={cap}: sum v L against X'(w r) of the applied step: {worst:.2e} of the bound")
    assert worst <= 1.0
    f.close()


# ---- the front ends ------------------------------------------------------------------------------------------------------------
def test_front_ends_after_a_fit():
    rng = np.random.default_rng(77)
    n, p = 300, 8
    X = np.asfortranarray(rng.standard_normal((n, p)))
    t = np.round(rng.exponential(1.0, n), 1) + 0.1
    status = (rng.random(n) < 0.7).astype(np.float64)
    g = 3 * rng.integers(0, 3, n) - 1
    v = rng.uniform(0.25, 4.0, n)
    off = rng.uniform(-0.3, 0.3, n)
    cluster = rng.integers(0, 40, n)
    f = cd.CDCoxLoss(np.c_[t, status], X, off, strata=g, weights=v)
    sol = cd.coxLasso(f, None, 0.2 * cd.coxLambdaMax(f))
    beta = sol.x.dense()
    sup = f._score_columns(None)                                  # the support in the handle's own order (cdh_get_support's)
    assert sol.converged and 1 <= len(sup) < p and np.array_equal(np.sort(sup), np.nonzero(beta)[0] + 1)
    eta_lin = f.y - f.r
    vn = f.weights
    L = f.score_residuals()
    assert L.shape == (n, len(sup))
    _, _, _, _, used = f._score(None, 50.0, info=True)           # the centres the device forms: the twin is given the same
    q = CSN.scan(X[:, sup - 1], eta_lin, off, t, status, 50.0, strata=g, weights=vn, centre=used)
    bs, bL, bI = _bounds(n, q)
    assert _worst(_err(L, q["score"]), bL) <= 1.0
    np.testing.assert_array_equal(cd.coxScoreResiduals(f), L)
    np.testing.assert_array_equal(f.score_residuals(weighted=True), L * vn[:, None])
    np.testing.assert_array_equal(f.score_residuals(sup), L)
    sch = f.schoenfeld_residuals()
    assert isinstance(sch, cd.CoxSchoenfeld) and np.array_equal(sch.columns, sup)
    ev = int(status.sum())
    assert sch.resid.shape == (ev, len(sup)) and sch.rows.shape == (ev,) and np.all(status[sch.rows] == 1.0)
    want_rows = np.array(sorted(np.nonzero(status)[0], key=lambda i: (g[i], t[i], i)))
    assert np.array_equal(sch.rows, want_rows) and np.array_equal(sch.stratum, g[want_rows]) and np.array_equal(sch.time, t[want_rows])
    assert _worst(_err(sch.resid, q["sch"][want_rows]), bs[want_rows]) <= 1.0
    np.testing.assert_array_equal(cd.coxSchoenfeldResiduals(f).resid, sch.resid)
    I = f.information()
    assert I.shape == (len(sup), len(sup)) and np.array_equal(I, I.T) and _worst(_err(I, q["info"]), bI) <= 1.0
    np.testing.assert_array_equal(cd.coxInformation(f), I)
    other = f.information([8, 1])
    assert other.shape == (2, 2) and other[0, 1] == other[1, 0]
    # Inference.  var = I^-1 and d var = -I^-1 dI I^-1 to first order, so in the 2-norm |d var| <= |I^-1|^2 |dI| = cond(I) |var|
    # (|dI| / |I|): the I bound (its Frobenius norm, which bounds |dI|_2) times the measured condition number, relative to
    # |var|_2, which every entry's error is below.  Both sides invert in float64: 8 m U cond more.  se_c = sqrt(var_cc):
    # d se_c = d var_cc / (2 se_c).
    want = CSN.inference(X[:, sup - 1], beta[sup - 1], eta_lin, off, t, status, g, vn, cluster)
    inf = cd.coxInference(f, robust=True, cluster=cluster)
    m = len(sup)
    cond = float(np.linalg.cond(want["info"]))
    relI = float(np.linalg.norm(bI) / np.linalg.norm(want["info"], 2))
    tol = cond * (relI + 8 * m * U)
    var2 = float(np.linalg.norm(want["var"], 2))
    print(f"cox score front ends: cond(I) = {cond:.3g}, relative I bound {relI:.3g}: tolerance of var {tol:.3g} of |var|_2; measured "
          f"{float(np.max(np.abs(inf.var - want['var']))) / var2:.3g}")
    assert np.array_equal(inf.columns, sup) and np.array_equal(inf.beta, beta[sup - 1])
    assert np.max(np.abs(inf.var - want["var"])) <= tol * var2
    assert np.all(np.abs(inf.se - want["se"]) <= tol * var2 / (2 * want["se"]))
    np.testing.assert_allclose(inf.z, beta[sup - 1] / inf.se, rtol=1e-15)
    # dfbeta_i = v_i L_i var, a row vector: d = v_i (dL_i var + L_i d var), every entry below the 2-norm,
    # v_i (|bL_i|_2 + |L_i|_2 tol) |var|_2, and the product's own rounding (m + 2) U v_i |L_i|_2 |var|_2.
    L2 = np.linalg.norm(q["score"].astype(np.float64), axis=1)
    bD = vn * (np.linalg.norm(bL, axis=1) + L2 * (tol + (m + 2) * U)) * var2
    assert np.all(np.abs(inf.dfbeta - want["dfbeta"]) <= bD[:, None])
    # D_k = the sum of dfbeta over cluster k: entries within bDk = the sum of its rows' bounds (and the sum's rounding, inside
    # the (m + 2) U above for clusters of a few rows).  robust_var = D'D: |d (D'D)_cd| <= sum_k (|D_kc| + |D_kd|) bDk, and the
    # product's rounding (K + 2) U sum_k |D_kc| |D_kd|; robust_se_c = sqrt: d / (2 robust_se_c).
    ids, inverse = np.unique(cluster, return_inverse=True)
    D, bDk = np.zeros((len(ids), m)), np.zeros(len(ids))
    np.add.at(D, inverse, want["dfbeta"])
    np.add.at(bDk, inverse, bD + n * U * np.abs(want["dfbeta"]).max(axis=1))
    Da = np.abs(D)
    bR = (Da.T @ bDk)[:, None] + (Da.T @ bDk)[None, :] + (len(ids) + 2) * U * (Da.T @ Da)
    assert np.all(np.abs(inf.robust_var - want["robust_var"]) <= bR)
    assert np.all(np.abs(inf.robust_se - want["robust_se"]) <= np.diag(bR) / (2 * want["robust_se"]))
    plain = cd.coxInference(f)
    assert plain.dfbeta is None and np.array_equal(plain.se, inf.se)
    # refusals of the front ends on a live handle
    empty = cd.SparseIterate(p)
    cd.initialize_(f, empty)
    with pytest.raises(cd.ArgumentError, match="support of β is empty"):
        f.score_residuals()
    f.set_ties("efron")
    with pytest.raises(cd.ArgumentError, match="not offered with Efron ties yet"):
        f.information([1, 2])
    f.close()
