"""The logistic lasso on the device: cdh_glm_set_labels, cdh_glm_irls (k_glm_step<GlmBinomial> -> k_gram_reduce) and the front ends on top of
them, held to the numpy twin (tests/_logistic_numpy.py; pinned against liblinear and the KKT conditions in
tests/test_glm_host.py).  The step is compared row by row at every edge of its plan (tests/_glm_plan.py, held to
csrc/glm_plan.hpp on the CPU), its sums on exactly summable values, its pad rows through the weighted moments, its
read-only form for leaving a cache-served handle alone, the state it leaves through solves on three kinds of handle and an
initialize! that must run, and the solves against the twin and against the KKT conditions of F itself.

Every case prints the figure it asserts on; LAB_NOTES.md "Logistic lasso" holds the ones measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _glm_plan as GP
import _logistic_numpy as LG

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
WRAP = GP.ROWS * GP.MAX_GRID                 # the first n whose tiles outnumber the full grid is WRAP + 1

# (n, grid cap, the branch the case is named for)
SHAPES = [(n, GP.MAX_GRID, "one short tile") for n in (1, 2, 3, 31, 32, 33)] + [
    (GP.ROWS - 1, GP.MAX_GRID, "one full tile"), (GP.ROWS, GP.MAX_GRID, "one full tile"), (GP.ROWS + 1, GP.MAX_GRID, "two workgroups"),
    (WRAP - 1, GP.MAX_GRID, "grid at its cap"), (WRAP, GP.MAX_GRID, "grid at its cap"), (WRAP + 1, GP.MAX_GRID, "second stride"),
    (2 * GP.ROWS, 2, "capped grid, one stride"), (2 * GP.ROWS + 1, 2, "second stride"), (5 * GP.ROWS + 7, 2, "third stride")]
IDS = ["n%d-cap%d" % (n, cap) for n, cap, _ in SHAPES]


def _reaches(n, cap, branch):
    pl = GP.plan(n, cap)
    want = {"one short tile": pl["tiles"] == 1 and pl["grid"] == 1 and pl["ld"] < GP.ROWS,
            "one full tile": pl["tiles"] == 1 and pl["ld"] == GP.ROWS,
            "two workgroups": pl["grid"] == 2 and pl["strides"] == 1,
            "grid at its cap": pl["grid"] == GP.MAX_GRID and pl["strides"] == 1,
            "capped grid, one stride": pl["grid"] == cap and pl["tiles"] == cap and pl["strides"] == 1,
            "second stride": pl["grid"] == cap and pl["strides"] == 2 and pl["tiles"] == cap + 1,
            "third stride": pl["grid"] == cap and pl["strides"] == 3}[branch]
    assert want, (n, cap, branch, pl)
    return pl


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _loss(monkeypatch, y, X, cap=GP.MAX_GRID):
    if cap != GP.MAX_GRID:
        monkeypatch.setenv("CDH_GLM_GRID", str(cap))          # read when the handle is made
    return cd.CDLogisticLoss(y, X)


def _irls(f, apply, wmin=1e-5):
    out = np.zeros(3)
    cd.check(f._L.cdh_glm_irls(f._h, int(apply), float(wmin), out.ctypes.data_as(C.POINTER(C.c_double))), f._h)
    return out


def _wmoments(f):
    sw, swr2 = C.c_double(), C.c_double()
    cd.check(f._L.cdh_resid_wmoments(f._h, C.byref(sw), C.byref(swr2)), f._h)
    return sw.value, swr2.value


# ---- the step, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,branch", SHAPES, ids=IDS)
def test_step_row_by_row(monkeypatch, n, cap, branch):
    """eta spread over about +-8 (wmin = 1e-3, so that the rows beyond |eta| = 6.9 clamp); each row against the twin's formulas
    at the eta the handle held: 64 ulp relative on w and r, 64 ulp of |eta| + |r| on z -- <= 2 ulp for the library's exp and
    log1p and fewer than ten rounded operations.  Measured on an MI355X: 5.4 / 5.7 / 4.0 ulp (w / r / z) at the worst."""
    _reaches(n, cap, branch)
    rng = np.random.default_rng(n)
    p, wmin = 3, 1e-3
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = (rng.random(n) < 0.5).astype(np.float64)
    f = _loss(monkeypatch, y, X, cap)
    x = cd.SparseIterate(p)
    x[1], x[2], x[3] = 2.5, -2.0, 1.5
    cd.initialize_(f, x)
    eta = f.y - f.r                                          # what the kernel recovers, from the same two stored vectors
    assert np.max(np.abs(eta)) > (6.0 if n > 30 else 0.0) and np.allclose(eta, X @ x.dense(), rtol=0, atol=1e-13)
    w_t, z_t, r_t, nll_t, cl_t = LG.rows(y, eta, wmin)
    ro = _irls(f, 0, wmin)
    out = _irls(f, 1, wmin)
    assert np.array_equal(ro, out)                           # the read-only form takes the same sums
    w, z, r = f.w, f.y, f.r
    ew, er = np.abs(w - w_t) / w_t, np.abs(r - r_t) / np.abs(r_t)
    ez = np.abs(z - z_t) / (np.abs(eta) + np.abs(r_t))
    print(f"step n={n} cap={cap}: worst ulps w {ew.max() / U:.2f} r {er.max() / U:.2f} z {ez.max() / U:.2f}, clamped {int(out[2])}")
    assert np.all(ew <= 64 * U) and np.all(er <= 64 * U) and np.all(ez <= 64 * U)
    assert out[2] == cl_t.sum() and (n < 1000 or out[2] > 0)
    assert abs(out[1] - w_t.sum()) <= (n + 64) * U * w_t.sum()
    assert abs(out[0] - nll_t.sum()) <= (n + 64) * U * np.abs(nll_t).sum()
    # the pad rows were written as zeros: the weighted moments over the handle's ld rows are those of the n real rows
    sw, swr2 = _wmoments(f)
    assert abs(sw - w.sum()) <= n * U * w.sum() and abs(swr2 - (w * r * r).sum()) <= 2 * n * U * (w * r * r).sum()
    f.close()


# ---- pads and exact sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,branch", SHAPES, ids=IDS)
def test_null_model_sums_are_exact_and_pads_are_zero(monkeypatch, n, cap, branch):
    """At beta = 0 straight after cdh_glm_set_labels every row has w = 1/4, r = +-2 and nll = log 2: sum w == n / 4 exactly,
    sum nll == n log 2 to 4 ulp; after the step sum w r^2 == n and the weighted column scales of an integer-valued X are exact.
    A pad row (eta = 0 there too) written as w = 1/4 instead of 0 shows in the first three.  Measured on an MI355X: sum nll
    off by 0 ulp up to n = 1024, 1 ulp on the capped grids, 4 / 4 / 3 ulp at n = 524 287 / 524 288 / 524 289 (1024 records)."""
    _reaches(n, cap, branch)
    rng = np.random.default_rng(n + 1)
    p = 2
    X = np.asfortranarray(rng.integers(-3, 4, size=(n, p)).astype(np.float64))
    y = (rng.random(n) < 0.5).astype(np.float64)
    f = _loss(monkeypatch, y, X, cap)
    np.testing.assert_array_equal(f.labels, y)
    np.testing.assert_array_equal(f.y, np.zeros(n))
    for apply in (0, 1):
        out = _irls(f, apply)
        want = n * np.log(2.0)
        print(f"null model n={n} cap={cap} apply={apply}: sum nll off by {abs(out[0] - want) / np.spacing(want):.2f} ulp")
        assert out[1] == n / 4 and out[2] == 0
        assert abs(out[0] - want) <= 4 * np.spacing(want)
    np.testing.assert_array_equal(f.w, np.full(n, 0.25))
    np.testing.assert_array_equal(f.r, 4.0 * y - 2.0)
    np.testing.assert_array_equal(f.y, 4.0 * y - 2.0)
    assert _wmoments(f) == (n / 4, float(n))
    np.testing.assert_array_equal(cd.stdX(f, weighted=True), np.sqrt(0.25 * (X * X).sum(axis=0) / n))
    # a second step from the same iterate (eta = z - r = 0 again) finds the same sums: nothing of the pad rows leaked in
    out2 = _irls(f, 1)
    assert out2[1] == n / 4 and abs(out2[0] - n * np.log(2.0)) <= 4 * np.spacing(n * np.log(2.0))
    assert _wmoments(f) == (n / 4, float(n))
    f.close()


# ---- read-only and determinism -------------------------------------------------------------------------------------------------
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


def test_read_only_step_leaves_a_cache_served_path_as_it_was():
    X, y, _ = LG.make_data(3000, 400, 10, 3)
    lmax = LG.lambda_max(X, y)
    opts = cd.CDOptions(maxIter=500, optTol=1e-12, randomize=False)
    f = cd.CDLogisticLoss(y, X)
    f.irls_step(True)                                        # one round's weighted lasso, solved along a path from the cache
    f.set_gradient_cache(2)
    cd.check(f._L.cdh_set_reuse_residual(f._h, 1), f._h)
    x = cd.SparseIterate(400)
    for frac in (0.8, 0.6, 0.45, 0.3):
        cd.coordinateDescent_(x, f, cd.ProxL1(frac * lmax), opts)
    assert f.cache_stats()["passes"] > 0 and x.nnz > 0                         # the cache is serving
    # the catch-up is cdh_loadings': a pending residual is brought up to date, and nothing else moves
    before = _snapshot(f)
    a = _irls(f, 0)
    after = _snapshot(f)
    _same(before, after, but=("residual_catchups",))
    assert 0 <= after["cache"]["residual_catchups"] - before["cache"]["residual_catchups"] <= 1
    # ... and with r up to date, nothing at all: twice the same bits, every counter, and r itself
    r0 = f.r
    before = _snapshot(f)
    b, c = _irls(f, 0), _irls(f, 0)
    after = _snapshot(f)
    assert np.array_equal(a, b) and np.array_equal(b, c)
    _same(before, after)
    np.testing.assert_array_equal(f.r, r0)
    eta = X @ x.dense()
    assert abs(b[0] - LG.rows(y, eta, 1e-5)[3].sum()) <= 1e-12 * b[0]           # F's own nll at the iterate, whatever z and w are
    assert f.objective() == b[0] / 3000
    # the path goes on from the cache as if nobody had looked
    passes = f.cache_stats()["passes"]
    cd.coordinateDescent_(x, f, cd.ProxL1(0.2 * lmax), opts)
    assert f.cache_stats()["passes"] > passes
    f.close()


# ---- the state a step leaves ---------------------------------------------------------------------------------------------------
KINDS = {"default": {}, "cache forced": {"CDH_GRADIENT_CACHE": "3"}, "one-launch": {"CDH_SMALL_PATH": "1"}}


def test_three_rounds_agree_on_three_kinds_of_handle(monkeypatch):
    """The same 3-round IRLS solve; a stale Gram matrix, X'Wz, z'Wz or stashed dot after a step shows as another beta."""
    n, p = 1000, 200
    X, y, _ = LG.make_data(n, p, 5, 3)
    lam = 0.1 * LG.lambda_max(X, y)
    opts = cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)
    want = LG.logistic_lasso(X, y, lam, maxIter=3, optTol=0.0)[0]
    got = {}
    for kind, env in KINDS.items():
        with monkeypatch.context() as m:                     # read when the handle is made; the suite's own setting comes back
            for k, v in env.items():
                m.setenv(k, v)
            f = cd.CDLogisticLoss(y, X)
        x = cd.SparseIterate(p)
        sol = cd.logisticLasso_(x, f, cd.ProxL1(lam), opts, cd.IRLSOptions(maxIter=3, optTol=0.0))
        assert sol.rounds == 3 and not sol.converged and sol.monotone
        got[kind] = x.dense()
        print(f"3 rounds [{kind}]: max|beta - twin| {np.max(np.abs(got[kind] - want)):.2e} cache {f.cache_stats()} onchip {f.onchip_stats()}")
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


def test_initialize_after_a_step_is_executed():
    """After a step r is consistent with the iterate but holds d / w, not fl(z - X beta): cdh_initialize must run.  r then is
    within the residual writers' bound 2 (M + L) 2^-53 A_i (tests/test_gpu_residual_writers.py: M = nnz + 1 operations,
    L = 1 store) of the long-double z - X beta, and bit for bit what a fresh weighted handle on (z, w) makes of the iterate."""
    n, p = 1537, 6
    rng = np.random.default_rng(9)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = (rng.random(n) < 0.5).astype(np.float64)
    f = cd.CDLogisticLoss(y, X)
    x = cd.SparseIterate(p)
    x[2], x[4], x[5] = 1.25, -0.75, 2.0
    cd.initialize_(f, x)
    f.irls_step(True)
    z, w, r_step = f.y, f.w, f.r
    cd.initialize_(f, x)
    r_init = f.r
    L_ = np.longdouble
    ref = z.astype(L_) - X.astype(L_) @ x.dense().astype(L_)
    A = np.abs(z) + np.abs(X) @ np.abs(x.dense())
    bound = 2.0 * ((3 + 1) + 1) * U * A
    assert np.all(np.abs(r_init.astype(L_) - ref) <= bound)
    assert not np.array_equal(r_init, r_step)                # d / w and fl(z - X beta) differ in their last bits somewhere
    g = cd.CDWeightedLSLoss(z, X, w)
    cd.initialize_(g, x)
    np.testing.assert_array_equal(r_init, g.r)
    # and the solve that follows is the fresh handle's
    opts = cd.CDOptions(maxIter=2000, optTol=1e-12, randomize=False)
    xa, xb = x.copy(), x.copy()
    cd.coordinateDescent_(xa, f, cd.ProxL1(0.05), opts)
    cd.coordinateDescent_(xb, g, cd.ProxL1(0.05), opts)
    assert xa.nnz > 0 and np.max(np.abs(xa.dense() - xb.dense())) <= 1e-11
    f.close()
    g.close()


# ---- solves --------------------------------------------------------------------------------------------------------------------
PROBLEMS = {"257x20": (257, 20, 3, 1, None), "500x50": (500, 50, 5, 2, None), "1000x200": (1000, 200, 5, 3, None),
            "intercept": (300, 12, 3, 7, 0.8)}
FRACS12 = np.geomspace(0.9, 0.05, 12)
_REF = {}


def _reference(name):
    """The twin's answers for a problem, computed once and shared by the ordered and the shuffled case."""
    if name not in _REF:
        n, p, s, seed, b0 = PROBLEMS[name]
        icpt = b0 is not None
        X, y, _ = LG.make_data(n, p, s, seed, b0 or 0.0)
        lmax = LG.lambda_max(X, y, intercept=icpt)
        one = LG.logistic_lasso(X, y, 0.1 * lmax, optTol=1e-10, intercept=icpt)
        warm = LG.logistic_lasso(X, y, 0.05 * lmax, optTol=1e-10, intercept=icpt,
                                 beta0=np.r_[one[0], one[1]] if icpt else one[0])
        sx = np.sqrt((X * X).sum(axis=0) / n)
        lmax_s = LG.lambda_max(X, y, sx, intercept=icpt)
        path = LG.logistic_path(X, y, FRACS12 * lmax_s, True, optTol=1e-10, intercept=icpt)
        _REF[name] = (X, y, lmax, one, warm, sx, lmax_s, path)
    return _REF[name]


def _kkt_ok(X, y, beta, lam, omega, b0, icpt):
    on, off, ic = LG.kkt(X, y, beta, lam, omega, b0)
    assert on <= 1e-8 and off <= 1e-8 and (not icpt or ic <= 1e-8), (on, off, ic)
    return max(on, off, ic if icpt else 0.0)


@pytest.mark.parametrize("randomize", (False, True), ids=("ordered", "shuffled"))
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_solves_against_the_twin_and_the_kkt_conditions(name, randomize):
    """logisticLasso, logisticLasso_ (warm) and LogisticLassoPath (12 lambda from 0.9 to 0.05 lambda_max); inner optTol 1e-12,
    IRLS optTol 1e-10.  beta against the twin at the project's 1e-10 (measured on an MI355X: 4.4e-13 at the largest); the KKT conditions
    of F evaluated in numpy from the returned beta at 1e-8, whatever the twin says; rounds <= 12, F never rising."""
    n, p, s, seed, b0 = PROBLEMS[name]
    icpt = b0 is not None
    X, y, lmax, one, warm, sx, lmax_s, path = _reference(name)
    opts = cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=randomize, seed=5)
    irls = cd.IRLSOptions(optTol=1e-10)
    worst = 0.0
    # the front end from a matrix
    sol = cd.logisticLasso(X, y, 0.1 * lmax, options=opts, irls=irls, fit_intercept=icpt)
    assert len(sol.x) == p and sol.converged and sol.monotone and sol.rounds <= 12 and (sol.intercept is not None) == icpt
    worst = max(worst, float(np.max(np.abs(sol.x.dense() - one[0]))), abs((sol.intercept or 0.0) - one[1]))
    _kkt_ok(X, y, sol.x.dense(), 0.1 * lmax, None, sol.intercept or 0.0, icpt)
    assert abs(sol.nll - (LG.objective(X, y, sol.x.dense(), 0.0, None, sol.intercept or 0.0))) <= 1e-13
    # lambda_max from the device, and the warm start on an existing loss
    X1 = LG.with_ones(X) if icpt else X
    f = cd.CDLogisticLoss(y, X1)
    assert abs(cd.logisticLambdaMax(f, fit_intercept=icpt) - lmax) <= 1e-13 * lmax
    om = np.r_[np.ones(p), 0.0] if icpt else None
    x = cd.SparseIterate(X1.shape[1], np.r_[one[0], one[1]] if icpt else one[0])
    sol = cd.logisticLasso_(x, f, cd.ProxL1(0.05 * lmax, om), opts, irls)
    beta = x.dense()
    assert sol.x is x and sol.converged and sol.monotone and sol.rounds <= 12
    worst = max(worst, float(np.max(np.abs(beta[:p] - warm[0]))), abs(beta[p] - warm[1]) if icpt else 0.0)
    _kkt_ok(X, y, beta[:p], 0.05 * lmax, None, beta[p] if icpt else 0.0, icpt)
    assert abs(cd.objective(f, cd.ProxL1(0.05 * lmax, om)) - LG.objective(X, y, beta[:p], 0.05 * lmax, None, beta[p] if icpt else 0.0)) <= 1e-13
    f.close()
    # the path
    res = cd.LogisticLassoPath(X, y, FRACS12 * lmax_s, opts, irls, fit_intercept=icpt)
    assert len(res.betapath) == 12 and len(res.nll) == 12 and max(res.rounds) <= 12 and all(res.converged)
    assert res.betapath[0].nnz >= 1 and res.betapath[-1].nnz > res.betapath[0].nnz
    for lam, b, bi, (tb, tb0, _) in zip(FRACS12 * lmax_s, res.betapath, res.intercepts, path):
        assert len(b) == p
        worst = max(worst, float(np.max(np.abs(b.dense() - tb))), abs((bi or 0.0) - tb0))
        _kkt_ok(X, y, b.dense(), lam, sx, bi or 0.0, icpt)
    print(f"solves [{name}, {'shuffled' if randomize else 'ordered'}]: max|beta_gpu - beta_twin| {worst:.2e}, path rounds {res.rounds}")
    assert worst <= 1e-10, worst


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    rng = np.random.default_rng(4)
    n, p = 50, 4
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = (rng.random(n) < 0.5).astype(np.float64)
    L = cd._lib.lib()
    out3 = np.zeros(3)
    po = out3.ctypes.data_as(C.POINTER(C.c_double))

    def refused(h, status):
        assert status == BAD and len(L.cdh_last_error(h)) > 0, (status, L.cdh_last_error(h))

    # a handle with labels: whatever is refused, labels, y, r, w and the sums stay
    f = cd.CDLogisticLoss(y, X)
    x = cd.SparseIterate(p)
    x[2] = 0.5
    cd.initialize_(f, x)
    f.irls_step(True)
    state = (f.labels, f.y, f.r, f.w, _irls(f, 0))
    for bad in (-0.1, 1.5, np.nan, np.inf):
        lab = y.copy()
        lab[17] = bad
        refused(f._h, L.cdh_glm_set_labels(f._h, 0, _vp(lab)))
        assert b"labels[17]" in L.cdh_last_error(f._h)
    for family in (1, -1, 7):
        refused(f._h, L.cdh_glm_set_labels(f._h, family, _vp(y)))
    refused(f._h, L.cdh_glm_set_labels(f._h, 0, None))
    refused(f._h, L.cdh_glm_get_labels(f._h, None))
    for wmin in (0.0, 0.3, -1e-5, np.nan):
        for apply in (0, 1):
            refused(f._h, L.cdh_glm_irls(f._h, apply, wmin, po))
    refused(f._h, L.cdh_glm_irls(f._h, 2, 1e-5, po))
    refused(f._h, L.cdh_glm_irls(f._h, 1, 1e-5, None))
    for a, b in zip(state, (f.labels, f.y, f.r, f.w, _irls(f, 0))):
        np.testing.assert_array_equal(a, b)
    assert L.cdh_glm_irls(f._h, 0, 0.25, po) == OK                              # the largest wmin allowed
    # on another loss the labels are refused and the handle goes on as the loss it is
    cd.check(L.cdh_set_loss(f._h, cd._lib.CDH_LS), f._h)
    refused(f._h, L.cdh_glm_irls(f._h, 0, 1e-5, po))
    refused(f._h, L.cdh_glm_set_labels(f._h, 0, _vp(y)))
    f.close()
    # NULL handles
    for status in (L.cdh_glm_set_labels(None, 0, _vp(y)), L.cdh_glm_get_labels(None, _vp(y)), L.cdh_glm_irls(None, 0, 1e-5, po)):
        refused(None, status)
    # irls and get_labels before labels
    g = cd.CDWeightedLSLoss(y, X, np.ones(n))
    refused(g._h, L.cdh_glm_irls(g._h, 1, 1e-5, po))
    refused(g._h, L.cdh_glm_get_labels(g._h, _vp(out3)))
    np.testing.assert_array_equal(g.y, y)
    g.close()
    # not CDH_WLS
    ls = cd.CDLeastSquaresLoss(y, X)
    refused(ls._h, L.cdh_glm_set_labels(ls._h, 0, _vp(y)))
    np.testing.assert_array_equal(ls.y, y)
    np.testing.assert_array_equal(ls.r, y)
    ls.close()
    # fp32 storage, and a row shard: refused, and still working handles
    y32 = y.astype(np.float32)
    for dtype, n_total, yy in ((cd._lib.CDH_F32, n, y32), (cd._lib.CDH_F64, 2 * n, y)):
        h = C.c_void_p()
        assert L.cdh_create(C.byref(h), dtype, cd._lib.CDH_WLS, n, n_total, 0, p, 0) == OK
        assert L.cdh_set_y(h, _vp(yy)) == OK
        refused(h, L.cdh_glm_set_labels(h, 0, _vp(y)))
        refused(h, L.cdh_glm_irls(h, 0, 1e-5, po))
        back = np.zeros_like(yy)
        assert L.cdh_get_y(h, _vp(back)) == OK and np.array_equal(back, yy)
        assert L.cdh_destroy(h) == OK
