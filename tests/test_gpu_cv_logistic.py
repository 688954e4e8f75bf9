"""Cross-validation of a logistic path on the device: cdh_glm_irls_fold (k_glm_step<GlmBinomialFold> -> k_gram_reduce) and cvLogisticLassoPath
on top of it, held to the numpy twins (tests/_logistic_numpy.py for the rows of a step, tests/_cv_logistic_numpy.py for the
folds: fitted on the training rows only, never as the masked formulation the product runs; tests/test_cv_logistic_host.py
pins both on the CPU).  The step is compared row by row on the shapes of tests/test_gpu_glm.py -- every edge of its plan
(tests/_glm_plan.py), odd n for the second row of the last vector, which has no fold id --, its sums on exactly summable values,
k = -1 bit for bit against cdh_glm_irls, its read-only form for leaving a cache-served handle alone, the state it leaves
through solves on three kinds of handle, the front end against the twin, and the refusals.

Every case prints the figure it asserts on; LAB_NOTES.md "Cross-validated logistic path" holds the ones measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cv_logistic_numpy as CL
import _cv_numpy as CV
import _glm_plan as GP
import _logistic_numpy as LG
from test_gpu_glm import IDS as GLM_IDS, SHAPES as GLM_SHAPES, _reaches

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
SHAPES = [s for s in GLM_SHAPES if s[0] >= 2]                # (one row cannot be split into a fold and its training rows)
IDS = [i for s, i in zip(GLM_SHAPES, GLM_IDS) if s[0] >= 2]
assert len(SHAPES) == len(GLM_SHAPES) - 1 and any(n % 2 for n, _, _ in SHAPES)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _loss(monkeypatch, y, X, cap=GP.MAX_GRID):
    if cap != GP.MAX_GRID:
        monkeypatch.setenv("CDH_GLM_GRID", str(cap))          # read when the handle is made
    return cd.CDLogisticLoss(y, X)


def _fold(f, k, apply, wmin=1e-5):
    out = np.zeros(5)
    cd.check(f._L.cdh_glm_irls_fold(f._h, int(k), int(apply), float(wmin), out.ctypes.data_as(C.POINTER(C.c_double))), f._h)
    return out


def _irls(f, apply, wmin=1e-5):
    out = np.zeros(3)
    cd.check(f._L.cdh_glm_irls(f._h, int(apply), float(wmin), out.ctypes.data_as(C.POINTER(C.c_double))), f._h)
    return out


def _wmoments(f):
    sw, swr2 = C.c_double(), C.c_double()
    cd.check(f._L.cdh_resid_wmoments(f._h, C.byref(sw), C.byref(swr2)), f._h)
    return sw.value, swr2.value


def _folds_of(n):
    """K = 3 and ids i % 3 (K = 2 and i % 2 at n = 2); the fold held out is 1."""
    K = 3 if n >= 3 else 2
    return K, (np.arange(n) % K).astype(np.int32), 1


# ---- the step, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,branch", SHAPES, ids=IDS)
def test_fold_step_row_by_row(monkeypatch, n, cap, branch):
    """The iterate and wmin of test_gpu_glm.py's test_step_row_by_row.  Training rows against the twin's formulas at its
    bounds (64 ulp relative on w and r, 64 ulp of |eta| + |r| on z); held-out rows w == 0, r == 0 and z == eta EXACTLY, eta
    as downloaded before the step; pad rows zero through the weighted moments; the counts exact; the three sums within
    (n + 64) 2^-53 of the twin's, relative to the sum of absolute values."""
    _reaches(n, cap, branch)
    rng = np.random.default_rng(n)
    p, wmin = 3, 1e-3
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = (rng.random(n) < 0.5).astype(np.float64)
    K, ids, k = _folds_of(n)
    held = ids == k
    f = _loss(monkeypatch, y, X, cap)
    f.set_folds(ids, K)
    x = cd.SparseIterate(p)
    x[1], x[2], x[3] = 2.5, -2.0, 1.5
    cd.initialize_(f, x)
    eta = f.y - f.r                                          # what the kernel recovers, from the same two stored vectors
    assert np.allclose(eta, X @ x.dense(), rtol=0, atol=1e-13)
    w_t, z_t, r_t, nll_t, cl_t = LG.rows(y, eta, wmin)
    miss_t = CL.miss(y, eta)
    ro = _fold(f, k, 0, wmin)
    out = _fold(f, k, 1, wmin)
    assert np.array_equal(ro, out)                           # the read-only form takes the same sums
    w, z, r = f.w, f.y, f.r
    tr = ~held
    ew, er = np.abs(w[tr] - w_t[tr]) / w_t[tr], np.abs(r[tr] - r_t[tr]) / np.abs(r_t[tr])
    ez = np.abs(z[tr] - z_t[tr]) / (np.abs(eta[tr]) + np.abs(r_t[tr]))
    print(f"fold step n={n} cap={cap}: worst ulps w {ew.max() / U:.2f} r {er.max() / U:.2f} z {ez.max() / U:.2f}, "
          f"clamped {int(out[2])}, held {int(held.sum())}, misclassified {int(out[4])}")
    assert np.all(ew <= 64 * U) and np.all(er <= 64 * U) and np.all(ez <= 64 * U)
    assert held.sum() >= 1 and tr.sum() >= 1
    np.testing.assert_array_equal(w[held], np.zeros(held.sum()))
    np.testing.assert_array_equal(r[held], np.zeros(held.sum()))
    np.testing.assert_array_equal(z[held], eta[held])
    assert out[2] == cl_t[tr].sum() and (n < 1000 or out[2] > 0)
    assert out[4] == miss_t[held].sum() and (n < 1000 or 0 < out[4] < held.sum())
    for got, terms in ((out[0], nll_t[tr]), (out[1], w_t[tr]), (out[3], nll_t[held])):
        assert abs(got - terms.sum()) <= (n + 64) * U * np.abs(terms).sum()
    # the pad rows were written as zeros: the weighted moments over the handle's ld rows are those of the n real rows
    sw, swr2 = _wmoments(f)
    assert abs(sw - w.sum()) <= n * U * w.sum() and abs(swr2 - (w * r * r).sum()) <= 2 * n * U * (w * r * r).sum()
    f.close()


# ---- exact sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,branch", SHAPES, ids=IDS)
def test_null_model_sums_of_a_fold_are_exact(monkeypatch, n, cap, branch):
    """At beta = 0 every training row has w = 1/4, r = +-2 and nll = log 2, every held-out row w = 0, z = 0 and nll = log 2, and
    eta = 0 predicts class 0: sum w == n_k / 4 and the misclassified count == the held-out ones exactly, the two nll sums to
    4 ulp, the weighted column scales of an integer-valued X exact.  A held-out row counted as training, a pad row counted at
    all, or a fold id read from the wrong byte shows in every one of them."""
    _reaches(n, cap, branch)
    rng = np.random.default_rng(n + 1)
    p = 2
    X = np.asfortranarray(rng.integers(-3, 4, size=(n, p)).astype(np.float64))
    y = (rng.random(n) < 0.5).astype(np.float64)
    K, ids, k = _folds_of(n)
    held = ids == k
    nk, size = int((~held).sum()), int(held.sum())
    f = _loss(monkeypatch, y, X, cap)
    f.set_folds(ids, K)
    outs = []
    for apply in (0, 1, 1):                                  # (the last: a second step from the same iterate, eta = z - r = 0 again)
        out = _fold(f, k, apply)
        outs.append(out)
        wt, wh = nk * np.log(2.0), size * np.log(2.0)
        print(f"null model of a fold n={n} cap={cap} apply={apply}: nll off by {abs(out[0] - wt) / np.spacing(wt):.2f} ulp (training) "
              f"{abs(out[3] - wh) / np.spacing(wh):.2f} ulp (held out)")
        assert out[1] == nk / 4 and out[2] == 0 and out[4] == y[held].sum()
        assert abs(out[0] - wt) <= 4 * np.spacing(wt) and abs(out[3] - wh) <= 4 * np.spacing(wh)
        if apply:
            np.testing.assert_array_equal(f.w, np.where(held, 0.0, 0.25))
            np.testing.assert_array_equal(f.r, np.where(held, 0.0, 4.0 * y - 2.0))
            np.testing.assert_array_equal(f.y, np.where(held, 0.0, 4.0 * y - 2.0))
            assert _wmoments(f) == (nk / 4, float(nk))
            np.testing.assert_array_equal(cd.stdX(f, weighted=True), np.sqrt(0.25 * (X[~held] * X[~held]).sum(axis=0) / n))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    f.close()


# ---- k = -1 is the plain step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", [(GP.ROWS + 1, GP.MAX_GRID), (2 * GP.ROWS + 1, 2)], ids=["n513", "n1025-cap2"])
def test_no_fold_is_the_plain_step_bit_for_bit(monkeypatch, n, cap):
    rng = np.random.default_rng(n)
    p, wmin = 3, 1e-3
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = (rng.random(n) < 0.5).astype(np.float64)
    fa, fb = _loss(monkeypatch, y, X, cap), _loss(monkeypatch, y, X, cap)
    x = cd.SparseIterate(p)
    x[1], x[2], x[3] = 2.5, -2.0, 1.5
    cd.initialize_(fa, x)
    cd.initialize_(fb, x)
    ro = _fold(fa, -1, 0, wmin)                              # no folds were ever set: a null table is accepted
    assert np.array_equal(ro[:3], _irls(fb, 0, wmin)) and ro[3] == 0.0 and ro[4] == 0.0
    for rounds in range(2):                                  # (the second from what the first wrote)
        a, b = _fold(fa, -1, 1, wmin), _irls(fb, 1, wmin)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] == 0.0 and a[4] == 0.0
        for u, v in ((fa.w, fb.w), (fa.y, fb.y), (fa.r, fb.r)):
            np.testing.assert_array_equal(u, v)
        assert _wmoments(fa) == _wmoments(fb)
    assert np.all(fa.w > 0)
    # ... and with folds set, k = -1 still holds nothing out
    fa.set_folds(np.arange(n) % 3, 3)
    assert np.array_equal(_fold(fa, -1, 0, wmin)[:3], _irls(fb, 0, wmin))
    fa.close()
    fb.close()


# ---- read-only -----------------------------------------------------------------------------------------------------------------
def _snapshot(f):
    beta, idx, nnz = np.zeros(f.p), np.zeros(f.p, dtype=np.int64), C.c_int64()
    cd.check(f._L.cdh_get_beta(f._h, _vp(beta)), f._h)
    cd.check(f._L.cdh_get_support(f._h, _vp(idx), C.byref(nnz)), f._h)
    return dict(cache=f.cache_stats(), onchip=f.onchip_stats(), beta=beta, sup=idx[: nnz.value].tolist(), w=f.w, y=f.y)


def _same(a, b, but=()):
    for k in ("beta", "w", "y"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["sup"] == b["sup"] and a["onchip"] == b["onchip"]
    assert {k: v for k, v in a["cache"].items() if k not in but} == {k: v for k, v in b["cache"].items() if k not in but}


def test_read_only_fold_step_leaves_a_cache_served_path_as_it_was():
    n, p, K, k = 3000, 400, 3, 1
    X, y, _ = LG.make_data(n, p, 10, 3)
    ids = CV.fold_ids(n, K, 0)
    held = ids == k
    lmax = LG.lambda_max(X, y)
    opts = cd.CDOptions(maxIter=500, optTol=1e-12, randomize=False)
    f = cd.CDLogisticLoss(y, X)
    f.set_folds(ids, K)
    f.irls_step(True, fold=k)                                # one round's weighted lasso of the fold, solved along a path from the cache
    f.set_gradient_cache(2)
    cd.check(f._L.cdh_set_reuse_residual(f._h, 1), f._h)
    x = cd.SparseIterate(p)
    for frac in (0.8, 0.6, 0.45, 0.3):
        cd.coordinateDescent_(x, f, cd.ProxL1(frac * lmax * (1 - held.mean())), opts)
    assert f.cache_stats()["passes"] > 0 and x.nnz > 0                         # the cache is serving
    np.testing.assert_array_equal(f.w[held], np.zeros(held.sum()))
    # the catch-up is cdh_loadings': a pending residual is brought up to date, and nothing else moves
    before = _snapshot(f)
    a = _fold(f, k, 0)
    after = _snapshot(f)
    _same(before, after, but=("residual_catchups",))
    assert 0 <= after["cache"]["residual_catchups"] - before["cache"]["residual_catchups"] <= 1
    # ... and with r up to date, nothing at all: twice the same bits, every counter, and r itself
    r0 = f.r
    before = _snapshot(f)
    b, c = _fold(f, k, 0), _fold(f, k, 0)
    after = _snapshot(f)
    assert np.array_equal(a, b) and np.array_equal(b, c)
    _same(before, after)
    np.testing.assert_array_equal(f.r, r0)
    eta = X @ x.dense()
    nll = LG.rows(y, eta, 1e-5)[3]
    assert abs(b[0] - nll[~held].sum()) <= 1e-12 * b[0] and abs(b[3] - nll[held].sum()) <= 1e-12 * b[3]
    assert b[4] == CL.miss(y, eta)[held].sum() and np.min(np.abs(eta[held])) > 1e-8
    # the held-out rows' linear predictor is where the next step looks for it
    np.testing.assert_allclose((f.y - f.r)[held], eta[held], rtol=0, atol=1e-12)
    # the path goes on from the cache as if nobody had looked
    passes = f.cache_stats()["passes"]
    cd.coordinateDescent_(x, f, cd.ProxL1(0.2 * lmax * (1 - held.mean())), opts)
    assert f.cache_stats()["passes"] > passes
    f.close()


# ---- the state a step leaves ---------------------------------------------------------------------------------------------------
KINDS = {"default": {}, "cache forced": {"CDH_GRADIENT_CACHE": "3"}, "one-launch": {"CDH_SMALL_PATH": "1"}}


def test_three_rounds_of_a_fold_agree_on_three_kinds_of_handle(monkeypatch):
    """The same 3-round IRLS solve of a fold, against the twin's three rounds on the training rows alone; a stale Gram matrix,
    X'Wz, z'Wz or stashed dot after a step, or a held-out row whose weight came back, shows as another beta."""
    n, p, K, k = 1000, 200, 3, 1
    X, y, _ = LG.make_data(n, p, 5, 3)
    ids = CV.fold_ids(n, K, 0)
    held = ids == k
    Xt, yt = np.asfortranarray(X[~held]), y[~held]
    nk = Xt.shape[0]
    lam = 0.1 * LG.lambda_max(X, y)
    opts = cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)
    want = LG.logistic_lasso(Xt, yt, lam, np.sqrt((Xt * Xt).sum(axis=0) / nk), maxIter=3, optTol=0.0)[0]
    assert np.count_nonzero(want) >= 3
    got = {}
    for kind, env in KINDS.items():
        with monkeypatch.context() as m:                     # read when the handle is made; the suite's own setting comes back
            for key, v in env.items():
                m.setenv(key, v)
            f = cd.CDLogisticLoss(y, X)
        f.set_folds(ids, K)
        f.set_fold_weights(k)
        sx = cd.stdX(f, weighted=True)
        x = cd.SparseIterate(p)
        sol = cd.logisticLasso_(x, f, cd.ProxL1(lam * np.sqrt(nk / n), sx), opts, cd.IRLSOptions(maxIter=3, optTol=0.0), fold=k)
        assert sol.rounds == 3 and not sol.converged and sol.monotone
        got[kind] = x.dense()
        eta = X @ got[kind]
        assert abs(sol.held_nll - LG.rows(y, eta, 0.25)[3][held].sum()) <= 1e-9 * sol.held_nll
        assert sol.held_miss == CL.miss(y, eta)[held].sum()
        np.testing.assert_array_equal(f.w[held], np.zeros(held.sum()))
        print(f"3 rounds of a fold [{kind}]: max|beta - twin| {np.max(np.abs(got[kind] - want)):.2e} cache {f.cache_stats()} "
              f"onchip {f.onchip_stats()}")
        if kind == "one-launch":
            assert f.onchip_stats()["solves"] >= 3
        else:
            assert f.onchip_stats()["solves"] == 0
        if kind == "cache forced":
            assert f.gradient_cache_mode() == 3
        f.close()
    for kind in KINDS:
        assert np.max(np.abs(got[kind] - want)) <= 1e-10, kind
        assert np.max(np.abs(got[kind] - got["default"])) <= 1e-10, kind


# ---- the front end -------------------------------------------------------------------------------------------------------------
def _opts(randomize):
    return cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=randomize, seed=5)


@pytest.mark.parametrize("name,randomize", [("257x20", False), ("300x12+b", False), ("500x50", False), ("500x50", True)],
                         ids=["257x20-ordered", "300x12+b-ordered", "500x50-ordered", "500x50-shuffled"])
def test_cv_logistic_path_against_the_twin(name, randomize):
    """12 lambda from 0.9 to 0.02 of lambda_max; inner optTol 1e-12, IRLS optTol 1e-10.  Every coefficient and intercept of
    every fold's path within the project's 1e-10 of the twin's fit on the training rows alone; the deviances within 1e-9
    relative; the class errors EXACTLY (entries with a held-out |eta| below 1e-8 in the twin are left out, at most 2 of
    them); the selections of both measures; `path` bit for bit LogisticLassoPath on all rows."""
    X, y, icpt, K, ids, lams = CL.data(name)
    t = CL.cv(name)
    p, m = X.shape[1], len(lams)
    irls = cd.IRLSOptions(optTol=1e-10)
    res = cd.cvLogisticLassoPath(X, y, lams, K=K, options=_opts(randomize), irls=irls, fit_intercept=icpt, keep_fold_paths=True)
    assert isinstance(res, cd.CVLogisticLassoPathResult) and res.measure == "deviance"
    np.testing.assert_array_equal(res.fold_sizes, t["sizes"])
    np.testing.assert_array_equal(res.lambdapath, lams)
    assert res.fold_deviance.shape == res.train_deviance.shape == res.fold_class.shape == res.rounds.shape == res.converged.shape == (K, m)
    assert res.converged.all() and res.rounds.max() <= 12 and res.rounds.min() >= 1
    worst = 0.0
    assert len(res.fold_paths) == K
    for k in range(K):
        fp = res.fold_paths[k]
        assert len(fp.betapath) == m and len(fp.intercepts) == m and fp.rounds == res.rounds[k].tolist()
        for b, bi, (tb, tb0, _) in zip(fp.betapath, fp.intercepts, t["paths"][k]):
            assert len(b) == p and (bi is not None) == icpt
            worst = max(worst, float(np.max(np.abs(b.dense() - tb))), abs((bi or 0.0) - tb0))
    edev = float(np.max(np.abs(res.fold_deviance - t["fold_deviance"]) / t["fold_deviance"]))
    etdev = float(np.max(np.abs(res.train_deviance - t["train_deviance"]) / t["train_deviance"]))
    decided = t["min_abs_eta"] >= 1e-8
    print(f"cv logistic path [{name}, {'shuffled' if randomize else 'ordered'}]: max|beta_gpu - beta_twin| {worst:.2e}, deviance rel "
          f"{edev:.2e} (held out) {etdev:.2e} (training), undecided class entries {int((~decided).sum())}, "
          f"index_min {res.index_min} index_1se {res.index_1se}, rounds {int(res.rounds.sum())}")
    assert worst <= 1e-10, worst
    assert edev <= 1e-9 and etdev <= 1e-9
    assert (~decided).sum() <= 2
    np.testing.assert_array_equal(res.fold_class[decided], t["fold_class"][decided])
    # the selections, by both measures
    cvm, cvsd, imin, i1se = t["deviance"]
    assert (res.index_min, res.index_1se) == (imin, i1se) and imin == CL.INDEX_MIN[name]
    assert res.lambda_min == lams[imin] and res.lambda_1se == lams[i1se]
    np.testing.assert_allclose(res.cvm, cvm, rtol=1e-9)
    np.testing.assert_allclose(res.cvsd, cvsd, rtol=1e-6)
    byc = cd.cvLogisticLassoPath(X, y, lams, K=K, options=_opts(randomize), irls=irls, fit_intercept=icpt, measure="class",
                                 full_path=False)
    assert byc.path is None and byc.fold_paths is None and byc.measure == "class"
    np.testing.assert_array_equal(byc.fold_class, res.fold_class)
    ccvm, ccvsd, cimin, ci1se = t["class"]
    if decided.all():
        np.testing.assert_allclose(byc.cvm, ccvm, rtol=1e-13)
        if np.sum(ccvm == ccvm.min()) == 1:
            assert (byc.index_min, byc.index_1se) == (cimin, ci1se)
    # the path on all rows is what LogisticLassoPath makes of a fresh handle, bit for bit
    ref = cd.LogisticLassoPath(X, y, lams, _opts(randomize), irls, fit_intercept=icpt)
    assert res.path.rounds == ref.rounds and res.path.intercepts == ref.intercepts and res.path.nll == ref.nll
    for a, b in zip(res.path.betapath, ref.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())
        assert a.nzval2ind.tolist() == b.nzval2ind.tolist()


def test_a_loss_that_was_passed_in_comes_back_without_folds():
    X, y, icpt, K, ids, lams = CL.data("257x20")
    t = CL.cv("257x20")
    f = cd.CDLogisticLoss(y, X)
    mode = f.gradient_cache_mode()
    res = cd.cvLogisticLassoPath(f, None, lams, K=K, options=_opts(False), irls=cd.IRLSOptions(optTol=1e-10), standardizeX=True)
    assert (res.index_min, res.index_1se) == t["deviance"][2:] and f.gradient_cache_mode() == mode
    np.testing.assert_array_equal(res.fold_class, t["fold_class"])
    # the handle's weights are what a plain step writes -- no zeros: the path on all rows ran last -- and the folds are gone
    assert np.all(f.w > 0) and len(res.path.betapath) == len(lams)
    last = res.path.betapath[-1].dense()
    np.testing.assert_allclose(f.w, LG.rows(y, X @ last, 1e-5)[0], rtol=1e-6)
    out = np.zeros(5)
    assert f._L.cdh_glm_irls_fold(f._h, 0, 0, 1e-5, out.ctypes.data_as(C.POINTER(C.c_double))) == BAD
    assert b"cdh_set_folds" in f._L.cdh_last_error(f._h)
    # without standardising the scales are ones and lambda n_k / n: the same training-rows-only fit of an unstandardised path
    k = 0
    held = ids == k
    Xt, yt = np.asfortranarray(X[~held]), y[~held]
    lam2 = lams[[2, 5]] * 1.5
    un = cd.cvLogisticLassoPath(f, None, lam2, K=K, options=_opts(False), irls=cd.IRLSOptions(optTol=1e-10), standardizeX=False,
                                full_path=False, keep_fold_paths=True)
    want = LG.logistic_path(Xt, yt, lam2, False, optTol=1e-10)
    for b, (tb, _, _) in zip(un.fold_paths[k].betapath, want):
        assert np.count_nonzero(tb) >= 1 and np.max(np.abs(b.dense() - tb)) <= 1e-10
    f.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    rng = np.random.default_rng(4)
    n, p, K = 50, 4, 3
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = (rng.random(n) < 0.5).astype(np.float64)
    L = cd._lib.lib()
    out5 = np.zeros(5)
    po = out5.ctypes.data_as(C.POINTER(C.c_double))

    def refused(h, status, word=None):
        assert status == BAD and len(L.cdh_last_error(h)) > 0, (status, L.cdh_last_error(h))
        assert word is None or word in L.cdh_last_error(h), (word, L.cdh_last_error(h))

    f = cd.CDLogisticLoss(y, X)
    x = cd.SparseIterate(p)
    x[2] = 0.5
    cd.initialize_(f, x)
    # k >= 0 without folds
    for apply in (0, 1):
        refused(f._h, L.cdh_glm_irls_fold(f._h, 0, apply, 1e-5, po), b"needs cdh_set_folds first")
    f.set_folds(np.arange(n) % K, K)
    _fold(f, 1, 1)
    state = (f.labels, f.y, f.r, f.w, _fold(f, 1, 0))
    assert np.count_nonzero(f.w == 0.0) == np.count_nonzero(np.arange(n) % K == 1)
    for apply in (0, 1):
        refused(f._h, L.cdh_glm_irls_fold(f._h, -2, apply, 1e-5, po), b"k must be a fold")
        refused(f._h, L.cdh_glm_irls_fold(f._h, K, apply, 1e-5, po), b"below the K")
        refused(f._h, L.cdh_glm_irls_fold(f._h, 255, apply, 1e-5, po), b"below the K")
        for wmin in (0.0, 0.3, -1e-5, np.nan):
            refused(f._h, L.cdh_glm_irls_fold(f._h, 1, apply, wmin, po), b"wmin")
        refused(f._h, L.cdh_glm_irls_fold(f._h, 1, apply, 1e-5, None))
    refused(f._h, L.cdh_glm_irls_fold(f._h, 1, 2, 1e-5, po), b"apply")
    # an exchange installed makes the handle a row shard: refused, and accepted again when it is gone
    f.set_host_exchange(lambda buf: None, 0, 1)
    for apply in (0, 1):
        refused(f._h, L.cdh_glm_irls_fold(f._h, 1, apply, 1e-5, po), b"row-sharded")
    f.set_host_exchange(None, 0, 1)
    for a, b in zip(state, (f.labels, f.y, f.r, f.w, _fold(f, 1, 0))):
        np.testing.assert_array_equal(a, b)
    assert L.cdh_glm_irls_fold(f._h, K - 1, 0, 0.25, po) == OK                  # the last fold, the largest wmin allowed
    # a least-squares handle: refused, with labels and folds still in it
    cd.check(L.cdh_set_loss(f._h, cd._lib.CDH_LS), f._h)
    refused(f._h, L.cdh_glm_irls_fold(f._h, 1, 0, 1e-5, po), b"CDH_WLS")
    f.close()
    # a NULL handle
    assert L.cdh_glm_irls_fold(None, 0, 0, 1e-5, po) == BAD
    # a weighted handle without labels
    g = cd.CDWeightedLSLoss(y, X, np.ones(n))
    g.set_folds(np.arange(n) % K, K)
    refused(g._h, L.cdh_glm_irls_fold(g._h, 1, 1, 1e-5, po), b"cdh_glm_set_labels")
    np.testing.assert_array_equal(g.y, y)
    np.testing.assert_array_equal(g.w, np.ones(n))
    g.close()
    # fp32 storage: refused, and still a working handle
    y32 = y.astype(np.float32)
    h = C.c_void_p()
    assert L.cdh_create(C.byref(h), cd._lib.CDH_F32, cd._lib.CDH_WLS, n, n, 0, p, 0) == OK
    assert L.cdh_set_y(h, _vp(y32)) == OK
    refused(h, L.cdh_glm_irls_fold(h, -1, 0, 1e-5, po), b"fp64")
    back = np.zeros_like(y32)
    assert L.cdh_get_y(h, _vp(back)) == OK and np.array_equal(back, y32)
    assert L.cdh_destroy(h) == OK
