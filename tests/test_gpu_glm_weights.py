"""Observation weights of the logistic and the Poisson lasso on the device: cdh_glm_set_weights, cdh_glm_get_weights and the
weighted instantiations of the step (k_glm_step<GlmBinomialFoldW>, k_glm_step<GlmPoissonW>) behind the three unchanged step
exports, with the front ends on top, held to the numpy twin (tests/_glm_weights_numpy.py; pinned in
tests/test_glm_weights_host.py).

The step is compared row by row with the UNWEIGHTED step of a second handle at the same iterate -- r and z with ==, w ==
v * w_unweighted with == -- at one vector, the odd live row, the pad rows, the 512-row tile edge on either side and, at
n = 1237, with workgroups that make several trips (CDH_GLM_GRID 1, 2, 3); the record against the twin within 64 U of the
sum of the terms' magnitudes (the magnitudes of the operands the row's term is formed from, v times test_gpu_poisson.py's
_scales).  Then unit weights, the fold step, the solves, lambda_max, the cross-validation against the twin's fits on the
training rows alone, the six front ends without weights on a handle that had them, and the refusals.

Every case prints the figure it asserts on; LAB_NOTES.md "Observation weights" holds the ones measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cv_numpy as CV
import _glm_plan as GP
import _glm_weights_numpy as GW
import _logistic_numpy as LG
import _poisson_numpy as PN

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
FAMILIES = ("binomial", "poisson")
WMIN, EMAX = 1e-3, 7.0                       # the rows below wmin clamp, the Poisson rows above eta_max cap

SHAPES = [(n, GP.MAX_GRID) for n in (1, 2, 31, 33, 511, 512, 513, 1237)] + [(1237, cap) for cap in (1, 2, 3)]
IDS = ["n%d-cap%d" % s for s in SHAPES]


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _case(family, n):
    """Rows whose eta_lin spreads over about +-8 (beta = (2.5, -2, 1.5)); labels in {0, 1}, or small counts with a non-constant
    offset in (-1, 1); log-uniform weights over [1e-3, 1e3]."""
    rng = np.random.default_rng(n)
    X = np.asfortranarray(rng.standard_normal((n, 3)))
    if family == "binomial":
        y, o = (rng.random(n) < 0.5).astype(np.float64), None
    else:
        y, o = rng.poisson(2.0, n).astype(np.float64), rng.uniform(-1.0, 1.0, n)
    v = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    x = cd.SparseIterate(3)
    x[1], x[2], x[3] = 2.5, -2.0, 1.5
    return X, y, o, v, x


def _loss(monkeypatch, family, y, X, o=None, v=None, cap=GP.MAX_GRID):
    if cap != GP.MAX_GRID:
        monkeypatch.setenv("CDH_GLM_GRID", str(cap))          # read when the handle is made
    return cd.CDLogisticLoss(y, X, weights=v) if family == "binomial" else cd.CDPoissonLoss(y, X, o, weights=v)


def _step(family, f, k, apply, wmin=WMIN, eta_max=EMAX):
    """The fold-aware export of the family: 5 or 6 sums."""
    po = C.POINTER(C.c_double)
    if family == "binomial":
        out = np.zeros(5)
        cd.check(f._L.cdh_glm_irls_fold(f._h, int(k), int(apply), float(wmin), out.ctypes.data_as(po)), f._h)
    else:
        out = np.zeros(6)
        cd.check(f._L.cdh_glm_poisson_irls(f._h, int(k), int(apply), float(wmin), float(eta_max), out.ctypes.data_as(po)), f._h)
    return out


def _irls3(f, apply, wmin=WMIN):
    out = np.zeros(3)
    cd.check(f._L.cdh_glm_irls(f._h, int(apply), float(wmin), out.ctypes.data_as(C.POINTER(C.c_double))), f._h)
    return out


def _set_weights(f, v):
    return f._L.cdh_glm_set_weights(f._h, _vp(v))


def _get_weights(f):
    out = np.zeros(f.n)
    cd.check(f._L.cdh_glm_get_weights(f._h, _vp(out)), f._h)
    return out


def _wmoments(f):
    sw, swr2 = C.c_double(), C.c_double()
    cd.check(f._L.cdh_resid_wmoments(f._h, C.byref(sw), C.byref(swr2)), f._h)
    return sw.value, swr2.value


def _magnitudes(family, y, eta_lin, o, v, held, wmin=WMIN, eta_max=EMAX):
    """Per entry of the record, the rows' magnitudes its error is relative to: v times the magnitudes of the operands the
    row's term is formed from (test_gpu_poisson.py's _scales: mu + |y ec| for the Poisson nll, y + mu for dev; max(eta, 0) +
    log1p(e) + |y eta| for the binomial nll), the stored w itself, and the terms themselves for the counts and v miss."""
    rec, terms = GW.record(family, y, eta_lin, o, v, held, wmin, eta_max)
    train = ~held
    if family == "binomial":
        s_nll = v * (np.maximum(eta_lin, 0.0) + np.log1p(np.exp(-np.abs(eta_lin))) + np.abs(y * eta_lin))
        mags = [np.where(train, s_nll, 0.0), terms[1], terms[2], np.where(held, s_nll, 0.0), terms[4]]
    else:
        ec = np.minimum(eta_lin + o, eta_max)
        mu = np.exp(ec)
        s_nll, s_dev = v * (mu + np.abs(y * ec)), v * (y + mu)
        mags = [np.where(train, s_nll, 0.0), terms[1], terms[2], terms[3], np.where(held, s_dev, 0.0), np.where(train, s_dev, 0.0)]
    return rec, mags


def _record_ok(tag, family, out, y, eta_lin, o, v, held):
    rec, mags = _magnitudes(family, y, eta_lin, o, v, held)
    counts = (2,) if family == "binomial" else (2, 3)
    worst = 0.0
    for i, (got, want, mag) in enumerate(zip(out, rec, mags)):
        if i in counts:
            assert got == want, (tag, i, got, want)
            continue
        worst = max(worst, abs(got - want) / (U * mag.sum()) if mag.sum() > 0 else abs(got - want))
        assert abs(got - want) <= 64 * U * mag.sum(), (tag, i, got, want, mag.sum())
    return worst


# ---- the step, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", SHAPES, ids=IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_weighted_step_row_by_row(monkeypatch, family, n, cap):
    """Two handles at one iterate, one with weights: r and z equal bit for bit, w == v * w_unweighted bit for bit (numpy's
    product is the one rounded multiplication), pad rows zero (the weighted moments over the handle's ld rows are those of
    the n rows), the read-only form takes the same sums, and the record is the twin's within 64 U of the sum of the terms'
    magnitudes, the counts exact.  The binomial family also through cdh_glm_irls: the first three sums of the fold-aware
    weighted step at k = -1, and the same rows."""
    pl = GP.plan(n, cap)
    assert (n != 1237) or pl["strides"] == {GP.MAX_GRID: 1, 1: 3, 2: 2, 3: 1}[cap]
    X, y, o, v_raw, x = _case(family, n)
    fu, fw = _loss(monkeypatch, family, y, X, o, None, cap), _loss(monkeypatch, family, y, X, o, v_raw, cap)
    v = fw.weights
    np.testing.assert_array_equal(v, cd.api._strata_weights(None, v_raw, n)[1])
    assert abs(v.sum() - n) <= 4 * n * U * n and (n < 30 or v.max() / v.min() > 1e3)
    np.testing.assert_array_equal(fu.weights, np.ones(n))
    for g in (fu, fw):
        cd.initialize_(g, x)
    eta = fw.y - fw.r
    np.testing.assert_array_equal(eta, fu.y - fu.r)
    nobody = np.zeros(n, dtype=bool)
    ro = _step(family, fw, -1, 0)
    out = _step(family, fw, -1, 1)
    plain = _step(family, fu, -1, 1)
    assert np.array_equal(ro, out)
    w, z, r = fw.w, fw.y, fw.r
    np.testing.assert_array_equal(r, fu.r)
    np.testing.assert_array_equal(z, fu.y)
    np.testing.assert_array_equal(w, v * fu.w)
    assert out[2] == plain[2] and (n < 1000 or out[2] > 0)                     # clamped: a row count, whatever v is
    if family == "poisson":
        assert out[3] == plain[3] and (n < 1000 or out[3] > 0)
    worst = _record_ok("step", family, out, y, eta, o, v, nobody)
    sw, swr2 = _wmoments(fw)
    assert abs(sw - w.sum()) <= n * U * w.sum() and abs(swr2 - (w * r * r).sum()) <= 2 * n * U * (w * r * r).sum()
    np.testing.assert_array_equal(fw.weights, v)                                # the weights are where they were
    print(f"weighted step [{family}] n={n} cap={cap}: r, z == and w == v w; record within {worst:.2f} U of its magnitudes")
    if family == "binomial":
        gw = _loss(monkeypatch, family, y, X, o, v_raw, cap)
        cd.initialize_(gw, x)
        ro3 = _irls3(gw, 0)
        assert gw.irls_step(False, WMIN)["nll"] == out[0] / n
        out3 = _irls3(gw, 1)
        assert np.array_equal(ro3, out[:3]) and np.array_equal(out3, out[:3])
        for a, b in ((gw.w, w), (gw.y, z), (gw.r, r)):
            np.testing.assert_array_equal(a, b)
        gw.close()
    fu.close()
    fw.close()


# ---- unit weights, and dropping them ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", [(33, GP.MAX_GRID), (513, GP.MAX_GRID), (1237, 2)], ids=["n33", "n513", "n1237-cap2"])
@pytest.mark.parametrize("family", FAMILIES)
def test_unit_weights_are_the_unweighted_step(monkeypatch, family, n, cap):
    """Ones through cdh_glm_set_weights run the weighted instantiation: w, y, r and the record of the unweighted step with ==
    (1 * t is t); NULL brings the handle back to the unweighted kernels, and cdh_glm_get_weights says ones either way."""
    X, y, o, _, x = _case(family, n)
    fu, fw = _loss(monkeypatch, family, y, X, o, None, cap), _loss(monkeypatch, family, y, X, o, None, cap)
    assert _set_weights(fw, np.ones(n)) == OK
    np.testing.assert_array_equal(_get_weights(fw), np.ones(n))
    for g in (fu, fw):
        cd.initialize_(g, x)
    for apply in (0, 1):
        assert np.array_equal(_step(family, fw, -1, apply), _step(family, fu, -1, apply))
    for a, b in ((fw.w, fu.w), (fw.y, fu.y), (fw.r, fu.r)):
        np.testing.assert_array_equal(a, b)
    # other weights, then NULL: the unweighted step again
    assert _set_weights(fw, np.full(n, 3.0)) == OK
    for g in (fu, fw):
        cd.initialize_(g, x)
    three = _step(family, fw, -1, 1)
    plain = _step(family, fu, -1, 1)
    np.testing.assert_array_equal(fw.w, 3.0 * fu.w)
    assert three[2] == plain[2] and abs(three[1] - 3.0 * plain[1]) <= 64 * U * three[1]
    assert _set_weights(fw, None) == OK
    np.testing.assert_array_equal(_get_weights(fw), np.ones(n))
    for g in (fu, fw):
        cd.initialize_(g, x)
    assert np.array_equal(_step(family, fw, -1, 1), _step(family, fu, -1, 1))
    for a, b in ((fw.w, fu.w), (fw.y, fu.y), (fw.r, fu.r)):
        np.testing.assert_array_equal(a, b)
    # a setter of observations drops the weights
    assert _set_weights(fw, np.full(n, 2.0)) == OK
    if family == "binomial":
        cd.check(fw._L.cdh_glm_set_labels(fw._h, 0, _vp(y)), fw._h)
    else:
        cd.check(fw._L.cdh_glm_set_counts(fw._h, _vp(y), _vp(o)), fw._h)
    np.testing.assert_array_equal(_get_weights(fw), np.ones(n))
    fu.close()
    fw.close()


# ---- the fold step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", [(2, GP.MAX_GRID), (33, GP.MAX_GRID), (513, GP.MAX_GRID), (1237, 3)],
                         ids=["n2", "n33", "n513", "n1237-cap3"])
@pytest.mark.parametrize("family", FAMILIES)
def test_fold_step_with_weights(monkeypatch, family, n, cap):
    """K = 3 (2 at n = 2), ids i % K, fold 1 held out; the Poisson family with its offset, so all five streams and the fold
    byte are read.  Held-out rows come back as (0, eta_lin, 0) EXACTLY, the training rows are the unfolded weighted step's
    bit for bit, the record is the twin's, and held + train is the all-rows sum (nll for the binomial family, deviance for
    the Poisson one) within 64 U of the sum of the terms' magnitudes; the weights round-trip."""
    X, y, o, v_raw, x = _case(family, n)
    K = 3 if n >= 3 else 2
    ids, k = (np.arange(n) % K).astype(np.int32), 1
    held = ids == k
    fa, fb = _loss(monkeypatch, family, y, X, o, v_raw, cap), _loss(monkeypatch, family, y, X, o, v_raw, cap)
    v = fa.weights
    fa.set_folds(ids, K)
    for g in (fa, fb):
        cd.initialize_(g, x)
    eta = fa.y - fa.r
    every = _step(family, fb, -1, 0)                          # no folds were ever set
    assert np.array_equal(_step(family, fa, -1, 0), every)
    ro = _step(family, fa, k, 0)
    out = _step(family, fa, k, 1)
    assert np.array_equal(ro, out)
    assert np.array_equal(_step(family, fb, -1, 1), every)
    w, z, r = fa.w, fa.y, fa.r
    np.testing.assert_array_equal(w[held], np.zeros(held.sum()))
    np.testing.assert_array_equal(r[held], np.zeros(held.sum()))
    np.testing.assert_array_equal(z[held], eta[held])
    for a, b in ((w, fb.w), (z, fb.y), (r, fb.r)):
        np.testing.assert_array_equal(a[~held], b[~held])
    worst = _record_ok("fold", family, out, y, eta, o, v, held)
    _, mags = _magnitudes(family, y, eta, o, v, np.zeros(n, dtype=bool))
    if family == "binomial":
        split, mag = abs((out[0] + out[3]) - every[0]), mags[0].sum()
        assert every[3] == 0.0 and every[4] == 0.0 and out[4] <= v[held].sum() * (1 + 64 * U)
    else:
        split, mag = abs((out[4] + out[5]) - every[5]), mags[5].sum()
        assert every[4] == 0.0 and out[3] == every[3]
    assert split <= 64 * U * mag
    sw, _ = _wmoments(fa)
    assert abs(sw - w.sum()) <= n * U * w.sum()               # pads zero
    np.testing.assert_array_equal(_get_weights(fa), v)
    # through the C ABI the weights are stored as given
    assert _set_weights(fa, v_raw) == OK
    np.testing.assert_array_equal(_get_weights(fa), v_raw)
    print(f"weighted fold step [{family}] n={n} cap={cap}: held {int(held.sum())}, record within {worst:.2f} U, "
          f"|held + train - all| {split / (U * mag):.2f} U of the magnitudes")
    fa.close()
    fb.close()


# ---- solves ----------------------------------------------------------------------------------------------------------------------
# name -> (family, n, p, planted coefficients, seed, intercept fitted?)
PROBLEMS = {"binomial 257x20": ("binomial", 257, 20, 3, 1, False), "binomial 300x12+b": ("binomial", 300, 12, 3, 7, True),
            "poisson 400x30+b": ("poisson", 400, 30, 5, 0, True), "poisson 500x20": ("poisson", 500, 20, 6, 2, False)}
FRACS = np.geomspace(0.7, 0.05, 5)
_REF = {}


def _opts():
    return cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)


def _problem(name):
    family, n, p, s, seed, icpt = PROBLEMS[name]
    if family == "binomial":
        X, y, _ = LG.make_data(n, p, s, seed, 0.8 if icpt else 0.0)
        o = None
    else:
        X, y, o, _ = PN.make_data(seed, n, p, s)
    return family, X, y, o, GW.weights(n, seed, 0.05, 20.0), icpt


def _reference(name):
    """The twin's answers for a problem, computed once: lambda_max (plain and standardised), one solve at 0.1 lambda_max and
    the standardised path at FRACS."""
    if name not in _REF:
        family, X, y, o, v, icpt = _problem(name)
        lmax = GW.lambda_max(family, X, y, o, v, None, icpt)
        one = GW.glm_lasso(family, X, y, o, v, 0.1 * lmax, optTol=1e-10, intercept=icpt)
        sx = np.sqrt((X * X).sum(axis=0) / X.shape[0])
        lmax_s = GW.lambda_max(family, X, y, o, v, sx, icpt)
        path = GW.glm_path(family, X, y, o, v, FRACS * lmax_s, True, optTol=1e-10, intercept=icpt)
        _REF[name] = (lmax, one, sx, lmax_s, path)
    return _REF[name]


def _front(family):
    if family == "binomial":
        return cd.CDLogisticLoss, cd.logisticLasso, cd.LogisticLassoPath, cd.cvLogisticLassoPath, cd.logisticLambdaMax
    return cd.CDPoissonLoss, cd.poissonLasso, cd.PoissonLassoPath, cd.cvPoissonLassoPath, cd.poissonLambdaMax


def _okw(family, o):
    return {} if family == "binomial" else {"offset": o}


def _kkt_ok(family, X, y, o, v, beta, lam, omega, b0, icpt):
    """|X_j'(v (y - mu))| / n <= lam omega_j, with equality and the sign on the support: from the host's data alone."""
    on, off, ic = GW.kkt(family, X, y, o, v, beta, lam, omega, b0)
    assert on <= 1e-8 and off <= 1e-8 and (not icpt or ic <= 1e-8), (on, off, ic)
    return max(on, off, ic if icpt else 0.0)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_weighted_solves_against_the_twin_and_the_kkt_conditions(name):
    """The family's lasso, lambda_max and path (5 lambda from 0.7 to 0.05 lambda_max, standardised by the UNWEIGHTED column
    rms) with weights over [0.05, 20] (normalised); inner optTol 1e-12, IRLS optTol 1e-10.  beta against the twin at the
    solve tests' 1e-10, the weighted KKT conditions in numpy at their 1e-8, lambda_max at the Poisson test's 1e-12 relative;
    the solve at lambda_max is null (to the rounding of the gradient's sum, below) and the one at 0.99 lambda_max is not."""
    family, X, y, o, v, icpt = _problem(name)
    lmax, one, sx, lmax_s, path = _reference(name)
    n, p = X.shape
    Loss, lasso, Path, _, lammax = _front(family)
    irls, kw = cd.IRLSOptions(optTol=1e-10), _okw(family, o)
    X1 = LG.with_ones(X) if icpt else X
    f = Loss(y, X1, weights=v) if family == "binomial" else Loss(y, X1, o, weights=v)
    np.testing.assert_array_equal(f.weights, v * n / v.sum())
    got = lammax(f, fit_intercept=icpt)
    got_s = lammax(f, np.r_[sx, 1.0][: f.p], fit_intercept=icpt)
    print(f"lambda_max [{name}]: device {got:.15g} twin {lmax:.15g} rel {abs(got - lmax) / lmax:.1e}")
    assert abs(got - lmax) <= 1e-12 * lmax and abs(got_s - lmax_s) <= 1e-12 * lmax_s
    nll0 = f.objective()
    assert abs(nll0 - GW.smooth(family, X, y, o, f.weights, np.zeros(p), GW.null_intercept(family, y, o, v) if icpt else 0.0)) <= 1e-12
    f.close()
    # At the device's own lambda_max the solve is null, at 0.99 of it it is not.  Null in floating point: the solver's
    # X_j'W r / n and lambda_max's are sums of the same n terms in another order, (n + 64) U apart relative to lambda_max at
    # most, so a coordinate whose |gradient| IS the maximum may move -- by that excess over its curvature d_j = X_j'W X_j / n
    # at the null model and no further (measured: 0 or 1.1e-16, run to run).
    vn = GW.normalise(v)
    b0 = GW.null_intercept(family, y, o, vn) if icpt else 0.0
    at = lasso(X, y, got, options=_opts(), irls=irls, fit_intercept=icpt, weights=v, **kw)
    below = lasso(X, y, 0.99 * got, options=_opts(), irls=irls, fit_intercept=icpt, weights=v, **kw)
    moved = float(np.max(np.abs(at.x.dense())))
    room = (n + 64) * U * got / GW.diagonal(family, X, y, o, vn, np.zeros(p), b0).min()
    print(f"    at lambda_max: nnz {at.x.nnz}, max|beta| {moved:.1e} (room {room:.1e}); at 0.99 of it: nnz {below.x.nnz}")
    assert moved <= room and at.x.nnz <= 1 and below.x.nnz >= 1 and at.converged and below.converged
    assert float(np.max(np.abs(below.x.dense()))) > 1e3 * room
    worst = 0.0
    sol = lasso(X, y, 0.1 * lmax, options=_opts(), irls=irls, fit_intercept=icpt, weights=v, **kw)
    assert len(sol.x) == p and sol.converged and (sol.intercept is not None) == icpt
    # (no step halving: from a cold start without an intercept the Poisson objective rises in the twin too -- by 0.57 on
    # "poisson 500x20" -- and the solution reports what the twin sees)
    assert sol.monotone == (one[4] <= 1e-10) and sol.rounds == one[2], (sol.monotone, one[4], sol.rounds, one[2])
    worst = max(worst, float(np.max(np.abs(sol.x.dense() - one[0]))), abs((sol.intercept or 0.0) - one[1]))
    _kkt_ok(family, X, y, o, vn, sol.x.dense(), 0.1 * lmax, None, sol.intercept or 0.0, icpt)
    assert abs(sol.nll - GW.smooth(family, X, y, o, vn, sol.x.dense(), sol.intercept or 0.0)) <= 1e-12
    lams = FRACS * lmax_s
    res = Path(X, y, lams, _opts(), irls, fit_intercept=icpt, weights=v, **kw)
    assert len(res.betapath) == 5 and all(res.converged) and res.betapath[-1].nnz > res.betapath[0].nnz >= 1
    for lam, b, bi, t in zip(lams, res.betapath, res.intercepts, path):
        worst = max(worst, float(np.max(np.abs(b.dense() - t[0]))), abs((bi or 0.0) - t[1]))
        _kkt_ok(family, X, y, o, vn, b.dense(), lam, sx, bi or 0.0, icpt)
    print(f"weighted solves [{name}]: max|beta_gpu - beta_twin| {worst:.2e}, rounds {sol.rounds}, path rounds {res.rounds}")
    assert worst <= 1e-10, worst


@pytest.mark.parametrize("family", FAMILIES)
def test_integer_weights_are_replicated_rows_on_the_device(family):
    """n = 40, p = 6, weights 1..3 against the same rows replicated (N = sum of the weights, unit weights), both through
    the device and both against the twin at the solve tests' 1e-10; the two nll agree at 1e-12."""
    X, y, o, _ = GW.make_data(family, 40, 6, 3, 3)
    reps = np.random.default_rng(3).integers(1, 4, 40)
    v = reps.astype(np.float64)
    Xr, yr, orr = GW.replicate(X, y, o, reps)
    lam = 0.2 * GW.lambda_max(family, X, y, o, GW.normalise(v))
    twin = GW.glm_lasso(family, X, y, o, GW.normalise(v), lam, optTol=1e-10)
    _, lasso, _, _, _ = _front(family)
    irls = cd.IRLSOptions(optTol=1e-10)
    a = lasso(X, y, lam, options=_opts(), irls=irls, weights=v, **_okw(family, o))
    b = lasso(Xr, yr, lam, options=_opts(), irls=irls, **_okw(family, orr))
    ea, eb = float(np.max(np.abs(a.x.dense() - twin[0]))), float(np.max(np.abs(b.x.dense() - twin[0])))
    print(f"replication on the device [{family}]: N = {len(yr)}, weighted {ea:.1e} replicated {eb:.1e} off the twin, "
          f"|nll_w - nll_r| {abs(a.nll - b.nll):.1e}")
    assert a.converged and b.converged and a.x.nnz >= 1
    assert ea <= 1e-10 and eb <= 1e-10 and abs(a.nll - b.nll) <= 1e-12


# ---- cross-validation ------------------------------------------------------------------------------------------------------------
_CV = {}


def _cv_data(family):
    X, y, o, v = GW.make_data(family, 180, 10, 4, 5, spread=(0.1, 10.0))
    return X, y, o, v


def _cv_twin(family, K, icpt, std):
    key = (family, K, icpt, std)
    if key not in _CV:
        X, y, o, v = _cv_data(family)
        sx = np.sqrt((X * X).sum(axis=0) / 180) if std else None
        lams = np.geomspace(0.8, 0.05, 5) * GW.lambda_max(family, X, y, o, v, sx, icpt)
        ids = CV.fold_ids(180, K, 0)
        _CV[key] = (lams, ids, GW.cv(family, X, y, o, v, lams, K, ids, icpt, std))
    return _CV[key]


@pytest.mark.parametrize("K,icpt,std", [(2, False, True), (3, True, True), (3, False, False), (2, True, False)],
                         ids=["K2-std", "K3-b-std", "K3-raw", "K2-b-raw"])
@pytest.mark.parametrize("family", FAMILIES)
def test_cv_path_with_weights_against_the_twin(family, K, icpt, std):
    """n = 180, p = 10, weights over [0.1, 10], 5 lambda from 0.8 to 0.05 of lambda_max; inner optTol 1e-12, IRLS optTol
    1e-10.  Every coefficient of every fold's path within the CV tests' 1e-10 of the twin's fit on the training rows ALONE
    with their weights renormalised, the deviances (and the weighted class error's cvm) within 1e-9 relative, cvm 1e-9 and
    cvsd 1e-6 as there; a selection is compared where the twin's own margin exceeds those tolerances; fold k's path within
    1e-10 of a fresh weighted path on X[train] through the device; `path` bit for bit the family's path with weights."""
    X, y, o, v = _cv_data(family)
    lams, ids, t = _cv_twin(family, K, icpt, std)
    p, m = X.shape[1], len(lams)
    _, _, Path, cvPath, _ = _front(family)
    irls, kw = cd.IRLSOptions(optTol=1e-10), _okw(family, o)
    res = cvPath(X, y, lams, K=K, folds=ids, options=_opts(), irls=irls, standardizeX=std, fit_intercept=icpt, weights=v,
                 keep_fold_paths=True, **kw)
    np.testing.assert_array_equal(res.fold_sizes, t["sizes"])
    assert res.converged.all() and res.rounds.max() <= 12
    worst = 0.0
    for k in range(K):
        fp = res.fold_paths[k]
        for b, bi, s in zip(fp.betapath, fp.intercepts, t["paths"][k]):
            assert len(b) == p and (bi is not None) == icpt
            worst = max(worst, float(np.max(np.abs(b.dense() - s[0]))), abs((bi or 0.0) - s[1]))
    edev = float(np.max(np.abs(res.fold_deviance - t["fold_deviance"]) / t["fold_deviance"]))
    etdev = float(np.max(np.abs(res.train_deviance - t["train_deviance"]) / t["train_deviance"]))
    cvm, cvsd, imin, i1se = t["deviance"]
    print(f"cv with weights [{family} K={K} intercept={icpt} standardize={std}]: max|beta_gpu - beta_twin| {worst:.2e}, "
          f"deviance rel {edev:.2e} (held out) {etdev:.2e} (training), index_min {res.index_min} index_1se {res.index_1se}")
    assert worst <= 1e-10, worst
    assert edev <= 1e-9 and etdev <= 1e-9
    np.testing.assert_allclose(res.cvm, cvm, rtol=1e-9)
    np.testing.assert_allclose(res.cvsd, cvsd, rtol=1e-6)
    rest = np.delete(cvm, imin)
    if rest.min() - cvm[imin] > 1e-8 * cvm[imin]:
        assert res.index_min == imin and res.lambda_min == lams[imin]
    bar = cvm[imin] + cvsd[imin]
    if res.index_min == imin and np.min(np.abs(cvm - bar)) > 1e-5 * bar:
        assert res.index_1se == i1se
    if family == "binomial":
        byc = cvPath(X, y, lams, K=K, folds=ids, options=_opts(), irls=irls, standardizeX=std, fit_intercept=icpt, weights=v,
                     measure="class", full_path=False)
        ecls = float(np.max(np.abs(byc.fold_class - t["fold_class"])))
        assert byc.path is None and ecls <= 1e-9 * max(1.0, t["fold_class"].max()) and byc.measure == "class"
        np.testing.assert_allclose(byc.cvm, t["class"][0], rtol=1e-9, atol=1e-12)
    # fold k's path against a fresh weighted path on the training rows, through the device
    k = K - 1
    tr = ids != k
    fresh = Path(np.asfortranarray(X[tr]), y[tr], lams, _opts(), irls, standardizeX=std, fit_intercept=icpt, weights=v[tr],
                 **_okw(family, None if o is None else o[tr]))
    wf = 0.0
    for b, bi, c, ci in zip(res.fold_paths[k].betapath, res.fold_paths[k].intercepts, fresh.betapath, fresh.intercepts):
        wf = max(wf, float(np.max(np.abs(b.dense() - c.dense()))), abs((bi or 0.0) - (ci or 0.0)))
    enll = max(abs(a - b) for a, b in zip(res.fold_paths[k].nll, fresh.nll))
    print(f"    fold {k} against a fresh weighted path on X[train]: {wf:.2e}, nll {enll:.1e}")
    assert wf <= 1e-10 and enll <= 1e-10
    # the path on all rows is what the family's path makes of a fresh handle with the same weights, bit for bit
    ref = Path(X, y, lams, _opts(), irls, standardizeX=std, fit_intercept=icpt, weights=v, **kw)
    assert res.path.rounds == ref.rounds and res.path.intercepts == ref.intercepts and res.path.nll == ref.nll
    for a, b in zip(res.path.betapath, ref.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())


# ---- without weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_without_weights_everything_is_as_it_was(family):
    """A handle that had weights set and then dropped (cdh_glm_set_weights(h, NULL)) against one that never had any: a step,
    lambda_max and the family's three front ends on the loss give the same bits; and from a matrix weights=None is the call
    of before."""
    X, y, o, v = GW.make_data(family, 150, 8, 3, 9)
    Loss, lasso, Path, cvPath, lammax = _front(family)
    irls = cd.IRLSOptions(optTol=1e-10)
    make = (lambda: Loss(y, X)) if family == "binomial" else (lambda: Loss(y, X, o))
    fa, fb = make(), make()
    assert _set_weights(fb, v) == OK
    x = cd.SparseIterate(8)
    x[2] = 0.3
    cd.initialize_(fb, x)
    _step(family, fb, -1, 1)                                  # the weighted kernel has run on it
    assert _set_weights(fb, None) == OK
    la, lb = lammax(fa), lammax(fb)
    assert la == lb
    for g in (fa, fb):
        cd.initialize_(g, x)
    assert np.array_equal(_step(family, fa, -1, 1), _step(family, fb, -1, 1))
    for a, b in ((fa.w, fb.w), (fa.y, fb.y), (fa.r, fb.r)):
        np.testing.assert_array_equal(a, b)
    lams = np.geomspace(0.6, 0.1, 3) * la
    sa, sb = lasso(fa, None, 0.2 * la, options=_opts(), irls=irls), lasso(fb, None, 0.2 * la, options=_opts(), irls=irls)
    assert sa.nll == sb.nll and sa.rounds == sb.rounds and sa.x.nnz >= 1
    np.testing.assert_array_equal(sa.x.dense(), sb.x.dense())
    pa, pb = Path(fa, None, lams, _opts(), irls), Path(fb, None, lams, _opts(), irls)
    assert pa.nll == pb.nll and pa.rounds == pb.rounds
    for a, b in zip(pa.betapath, pb.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())
    ca = cvPath(fa, None, lams, K=3, options=_opts(), irls=irls, keep_fold_paths=True)
    cb = cvPath(fb, None, lams, K=3, options=_opts(), irls=irls, keep_fold_paths=True)
    for name in ("fold_deviance", "train_deviance", "cvm", "cvsd", "rounds"):
        np.testing.assert_array_equal(getattr(ca, name), getattr(cb, name))
    assert (ca.index_min, ca.index_1se) == (cb.index_min, cb.index_1se) and ca.path.nll == cb.path.nll
    for k in range(3):
        for a, b in zip(ca.fold_paths[k].betapath, cb.fold_paths[k].betapath):
            np.testing.assert_array_equal(a.dense(), b.dense())
    fa.close()
    fb.close()
    # from a matrix: weights=None, and unit weights at the solve tolerance (another kernel, the same minimiser)
    kw = _okw(family, o)
    m0 = lasso(X, y, 0.2 * la, options=_opts(), irls=irls, **kw)
    m1 = lasso(X, y, 0.2 * la, options=_opts(), irls=irls, weights=None, **kw)
    m2 = lasso(X, y, 0.2 * la, options=_opts(), irls=irls, weights=np.full(150, 7.0), **kw)
    assert m0.nll == m1.nll == sa.nll
    np.testing.assert_array_equal(m0.x.dense(), m1.x.dense())
    assert np.max(np.abs(m2.x.dense() - m0.x.dense())) <= 1e-10


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    n = 33
    X, y, o, v_raw, x = _case("poisson", n)
    L = cd._lib.lib()

    def refused(f, status, *words):
        assert status == BAD
        msg = L.cdh_last_error(f._h)
        for w in words:
            assert w in msg, (w, msg)

    f = cd.CDPoissonLoss(y, X, o, weights=v_raw)
    v = f.weights
    cd.initialize_(f, x)
    before = _step("poisson", f, -1, 0)
    for bad, at in ((np.nan, 0), (np.inf, n - 1), (-np.inf, 5), (0.0, 7), (-1.0, 32), (-5e-324, 1)):
        u = v_raw.copy()
        u[at] = bad
        refused(f, _set_weights(f, u), b"weights[%d]" % at, b"not finite and > 0")
        np.testing.assert_array_equal(_get_weights(f), v)
        assert np.array_equal(_step("poisson", f, -1, 0), before)
    refused(f, L.cdh_glm_get_weights(f._h, None), b"NULL")
    u = v_raw.copy()
    u[3] = 5e-324                                             # a denormal is a weight like any other
    assert _set_weights(f, u) == OK
    np.testing.assert_array_equal(_get_weights(f), u)
    f.close()
    # a Cox handle: its weights come through cdh_glm_set_survival_strata, and stay
    t = np.c_[np.arange(1.0, n + 1), (np.arange(n) % 2 == 0).astype(float)]
    g = cd.CDCoxLoss(t, X, weights=v_raw)
    gv = g.weights
    refused(g, _set_weights(g, v_raw), b"cdh_glm_set_survival_strata")
    refused(g, _set_weights(g, None), b"cdh_glm_set_survival_strata")
    out = np.zeros(n)
    refused(g, L.cdh_glm_get_weights(g._h, _vp(out)), b"cdh_glm_get_survival_strata")
    np.testing.assert_array_equal(g.weights, gv)
    g.close()
    # a handle without observations
    h = cd.CDWeightedLSLoss(y, X, np.ones(n))
    refused(h, _set_weights(h, v_raw), b"cdh_glm_set_labels")
    refused(h, L.cdh_glm_get_weights(h._h, _vp(out)), b"cdh_glm_set_labels")
    np.testing.assert_array_equal(h.w, np.ones(n))
    h.close()
    # NULL handles
    assert L.cdh_glm_set_weights(None, _vp(v_raw)) == BAD and b"NULL" in L.cdh_last_error(None)
    assert L.cdh_glm_get_weights(None, _vp(out)) == BAD and b"NULL" in L.cdh_last_error(None)
    # a binomial handle with weights made Poisson, and a Poisson one made Cox: the weights go with the observations
    b = cd.CDLogisticLoss((y > 1).astype(float), X, weights=v_raw)
    cd.check(L.cdh_glm_set_counts(b._h, _vp(y), None), b._h)
    np.testing.assert_array_equal(_get_weights(b), np.ones(n))
    assert _set_weights(b, v_raw) == OK
    cd.check(L.cdh_glm_set_survival(b._h, _vp(np.ascontiguousarray(t[:, 0])), _vp(np.ascontiguousarray(t[:, 1])), None), b._h)
    cd.check(L.cdh_glm_set_labels(b._h, 0, _vp((y > 1).astype(float))), b._h)
    np.testing.assert_array_equal(_get_weights(b), np.ones(n))
    b.close()
