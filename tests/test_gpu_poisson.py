"""The Poisson lasso on the device: cdh_glm_set_counts, cdh_glm_get_offset, cdh_glm_poisson_irls (k_glm_step<GlmPoisson> -> k_gram_reduce)
and the front ends on top of them, held to the numpy twin (tests/_poisson_numpy.py; pinned against L-BFGS-B and the KKT
conditions in tests/test_poisson_host.py).  The step is compared row by row at every edge of its plan (tests/_glm_plan.py:
the shapes of tests/test_gpu_glm.py restated), its sums on exactly summable values, its pad rows through the weighted moments,
the offset for staying out of the stored working response, the folds for weight zero on the held-out rows and for leaving the
training rows' bits alone, the read-only form for leaving a cache-served handle alone, the solves against the twin and against
the KKT conditions of F itself, the cross-validation against the twin's fits on the training rows alone, and the refusals.

Every case prints the figure it asserts on; LAB_NOTES.md "Poisson lasso" holds the ones measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cv_numpy as CV
import _glm_plan as GP
import _poisson_numpy as PN

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
FOLD_SHAPES = [s for s in SHAPES if s[0] >= 3]
FOLD_IDS = [i for s, i in zip(SHAPES, IDS) if s[0] >= 3]


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


def _loss(monkeypatch, y, X, o=None, cap=GP.MAX_GRID):
    if cap != GP.MAX_GRID:
        monkeypatch.setenv("CDH_GLM_GRID", str(cap))          # read when the handle is made
    return cd.CDPoissonLoss(y, X, o)


def _step(f, k, apply, wmin=1e-5, eta_max=50.0):
    out = np.zeros(6)
    cd.check(f._L.cdh_glm_poisson_irls(f._h, int(k), int(apply), float(wmin), float(eta_max),
                                       out.ctypes.data_as(C.POINTER(C.c_double))), f._h)
    return out


def _wmoments(f):
    sw, swr2 = C.c_double(), C.c_double()
    cd.check(f._L.cdh_resid_wmoments(f._h, C.byref(sw), C.byref(swr2)), f._h)
    return sw.value, swr2.value


def _row_case(n):
    """The data of the row-by-row cases: eta_lin = X beta spread over about +-8 (beta = (2.5, -2, 1.5)), a non-constant offset
    in (-1, 1), small counts."""
    rng = np.random.default_rng(n)
    X = np.asfortranarray(rng.standard_normal((n, 3)))
    y = rng.poisson(2.0, n).astype(np.float64)
    o = rng.uniform(-1.0, 1.0, n)
    x = cd.SparseIterate(3)
    x[1], x[2], x[3] = 2.5, -2.0, 1.5
    return X, y, o, x


def _scales(y, eta_lin, o, wmin, eta_max):
    """What the rows' rounding errors are relative to: mu for w; (y + mu) / w for r = (y - mu) / w, the subtraction of two
    non-negative numbers of which mu carries exp's error; |eta_lin| on top of that for z; mu + |y ec| for nll; y + mu for dev
    (a row's own error is a few (1 + |log(y / mu)|) ulp of that: at most a few tens, inside the 64 of a sum of one to three
    rows, where |log(y / mu)| <= 10, and far inside the n + 64 of the longer ones)."""
    ec = np.minimum(eta_lin + o, eta_max)
    mu = np.exp(ec)
    w = np.maximum(mu, wmin)
    return mu, (y + mu) / w, np.abs(eta_lin) + (y + mu) / w, mu + np.abs(y * ec), y + mu


# ---- the step, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,branch", SHAPES, ids=IDS)
def test_step_row_by_row(monkeypatch, n, cap, branch):
    """wmin = 1e-3 (the rows with mu below it clamp) and eta_max = 7 (the rows above it cap); each row against the twin's
    formulas at the eta_lin the handle held.  64 ulp on w relative to w, on r relative to (y + mu) / w and on z relative to
    |eta_lin| + (y + mu) / w: <= 2 ulp for the library's exp and fewer than ten rounded operations, as for the binomial step;
    unlike the binomial's d = y q - (1 - y) p, d = y - mu cancels, so r's error is relative to the operands of that
    subtraction, not to r.  The sums within (n + 64) 2^-53 of the twin's, relative to the sum of the rows' scales (_scales:
    dev cancels near y = mu, so its scale is y + mu).  The counts exact.  Measured on an MI355X: LAB_NOTES "Poisson lasso"."""
    _reaches(n, cap, branch)
    X, y, o, x = _row_case(n)
    wmin, emax = 1e-3, 7.0
    f = _loss(monkeypatch, y, X, o, cap)
    cd.initialize_(f, x)
    eta = f.y - f.r                                          # what the kernel recovers, from the same two stored vectors
    assert np.max(np.abs(eta)) > (6.0 if n > 30 else 0.0) and np.allclose(eta, X @ x.dense(), rtol=0, atol=1e-13)
    w_t, z_t, r_t, nll_t, dev_t, cl_t, cap_t = PN.rows(y, eta, o, wmin, emax)
    s_w, s_r, s_z, s_nll, s_dev = _scales(y, eta, o, wmin, emax)
    ro = _step(f, -1, 0, wmin, emax)
    out = _step(f, -1, 1, wmin, emax)
    assert np.array_equal(ro, out)                           # the read-only form takes the same sums, bit for bit
    w, z, r = f.w, f.y, f.r
    ew, er, ez = np.abs(w - w_t) / s_w, np.abs(r - r_t) / s_r, np.abs(z - z_t) / s_z
    nz = r_t != 0.0
    rel_r = (np.abs(r - r_t)[nz] / np.abs(r_t[nz])).max() if nz.any() else 0.0
    print(f"poisson step n={n} cap={cap}: worst ulps w {ew.max() / U:.2f} r {er.max() / U:.2f} z {ez.max() / U:.2f} "
          f"(r relative to |r| {rel_r / U:.1f}), clamped {int(out[2])} capped {int(out[3])}; sums off by "
          f"nll {abs(out[0] - nll_t.sum()) / (U * s_nll.sum()):.2f} w {abs(out[1] - w_t.sum()) / (U * s_w.sum()):.2f} "
          f"dev {abs(out[5] - dev_t.sum()) / (U * s_dev.sum()):.2f} ulp of their scales")
    assert np.all(ew <= 64 * U) and np.all(er <= 64 * U) and np.all(ez <= 64 * U)
    assert out[2] == cl_t.sum() and out[3] == cap_t.sum() and (n < 1000 or (out[2] > 0 and out[3] > 0))
    assert out[4] == 0.0                                     # nobody is held out
    for got, terms, scale in ((out[0], nll_t, s_nll), (out[1], w_t, s_w), (out[5], dev_t, s_dev)):
        assert abs(got - terms.sum()) <= (n + 64) * U * scale.sum()
    # the pad rows were written as zeros: the weighted moments over the handle's ld rows are those of the n real rows
    sw, swr2 = _wmoments(f)
    assert abs(sw - w.sum()) <= n * U * w.sum() and abs(swr2 - (w * r * r).sum()) <= 2 * n * U * (w * r * r).sum()
    # the counts and the offset are where they were
    np.testing.assert_array_equal(f.counts, y)
    np.testing.assert_array_equal(f.offset, o)
    f.close()


# ---- pads and exact sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,branch", SHAPES, ids=IDS)
def test_null_model_sums_are_exact_and_pads_are_zero(monkeypatch, n, cap, branch):
    """At beta = 0 without an offset, straight after cdh_glm_set_counts with counts in {0, 1}, every row has mu = w = 1,
    r = y - 1, nll = 1 and dev = 2 [y = 0]: sum w == n, sum nll == n and sum dev == 2 #{y = 0} EXACTLY; after the step
    sum w r^2 == #{y = 0} and the weighted column scales of an integer-valued X are exact.  A pad row (eta = 0 there too)
    written as w = 1 instead of 0 shows in all of them."""
    _reaches(n, cap, branch)
    rng = np.random.default_rng(n + 1)
    p = 2
    X = np.asfortranarray(rng.integers(-3, 4, size=(n, p)).astype(np.float64))
    y = (rng.random(n) < 0.5).astype(np.float64)
    zeros = float(np.sum(y == 0.0))
    f = _loss(monkeypatch, y, X, None, cap)
    np.testing.assert_array_equal(f.counts, y)
    np.testing.assert_array_equal(f.offset, np.zeros(n))
    np.testing.assert_array_equal(f.y, np.zeros(n))
    for apply in (0, 1, 1):                                  # (the last: a second step from the same iterate, eta = z - r = 0 again)
        out = _step(f, -1, apply)
        assert out.tolist() == [float(n), float(n), 0.0, 0.0, 0.0, 2.0 * zeros], (apply, out)
    np.testing.assert_array_equal(f.w, np.ones(n))
    np.testing.assert_array_equal(f.r, y - 1.0)
    np.testing.assert_array_equal(f.y, y - 1.0)
    assert _wmoments(f) == (float(n), zeros)
    np.testing.assert_array_equal(cd.stdX(f, weighted=True), np.sqrt((X * X).sum(axis=0) / n))
    f.close()


# ---- the offset ----------------------------------------------------------------------------------------------------------------
def test_offset_stays_out_of_the_working_response(monkeypatch):
    """After a step and a solve the stored y_w - r is X beta, not X beta + o; cdh_glm_get_offset round-trips; a null offset
    and an all-zero one give the same bits."""
    n = 2 * GP.ROWS + 1
    X, y, o, x = _row_case(n)
    x = cd.SparseIterate(3)
    x[1], x[3] = 0.3, -0.2
    f = _loss(monkeypatch, y, X, o + 2.0, 2)
    np.testing.assert_array_equal(f.offset, o + 2.0)
    cd.initialize_(f, x)
    f.irls_step(True)
    np.testing.assert_allclose(f.y - f.r, X @ x.dense(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(f.w, np.exp(X @ x.dense() + o + 2.0), rtol=1e-13)           # ... while mu has it
    check = cd.check
    check(f._L.cdh_set_reuse_residual(f._h, 1), f._h)
    cd.coordinateDescent_(x, f, cd.ProxL1(0.05), cd.CDOptions(maxIter=1000, optTol=1e-12, randomize=False))
    check(f._L.cdh_set_reuse_residual(f._h, 0), f._h)
    f.irls_step(False)                                       # (brings r up to date; reads only)
    assert x.nnz >= 1
    np.testing.assert_allclose(f.y - f.r, X @ x.dense(), rtol=0, atol=1e-13 * max(1.0, np.max(np.abs(f.y))))
    f.close()
    # null == zeros, bit for bit: the sums, and what the step writes
    fa, fb = _loss(monkeypatch, y, X, None, 2), _loss(monkeypatch, y, X, np.zeros(n), 2)
    np.testing.assert_array_equal(fa.offset, fb.offset)
    for g in (fa, fb):
        cd.initialize_(g, x)
    for apply in (0, 1, 1):
        assert np.array_equal(_step(fa, -1, apply, 1e-3, 7.0), _step(fb, -1, apply, 1e-3, 7.0))
    for u, v in ((fa.w, fb.w), (fa.y, fb.y), (fa.r, fb.r)):
        np.testing.assert_array_equal(u, v)
    # a second cdh_glm_set_counts without an offset drops the one the handle had
    cd.check(fb._L.cdh_glm_set_counts(fb._h, _vp(y), _vp(o)), fb._h)
    np.testing.assert_array_equal(fb.offset, o)
    cd.check(fb._L.cdh_glm_set_counts(fb._h, _vp(y), None), fb._h)
    np.testing.assert_array_equal(fb.offset, np.zeros(n))
    cd.check(fa._L.cdh_glm_set_counts(fa._h, _vp(y), None), fa._h)
    assert np.array_equal(_step(fa, -1, 1), _step(fb, -1, 1))
    fa.close()
    fb.close()


def test_constant_offset_moves_only_the_intercept():
    """o = c with a fitted intercept: the same beta, and the intercept minus c, as without an offset, to 10 x the IRLS optTol."""
    X, y, _, _ = PN.make_data(0)
    c, tol = 0.7, 1e-9
    lam = 0.2 * PN.lambda_max(X, y, None, intercept=True)
    opts, irls = cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False), cd.IRLSOptions(optTol=tol)
    a = cd.poissonLasso(X, y, lam, options=opts, irls=irls, fit_intercept=True)
    b = cd.poissonLasso(X, y, lam, options=opts, irls=irls, fit_intercept=True, offset=np.full(len(y), c))
    db, di = float(np.max(np.abs(a.x.dense() - b.x.dense()))), abs(a.intercept - c - b.intercept)
    print(f"constant offset: max|beta - beta_o| {db:.2e}, |b0 - c - b0_o| {di:.2e}, rounds {a.rounds} / {b.rounds}")
    assert a.converged and b.converged and a.x.nnz >= 3
    assert db <= 10 * tol and di <= 10 * tol


# ---- folds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,branch", FOLD_SHAPES, ids=FOLD_IDS)
def test_fold_step(monkeypatch, n, cap, branch):
    """K = 3, ids i % 3, fold 1 held out.  Held-out rows come back as (0, eta_lin, 0) EXACTLY; the training rows are the
    unfolded step's rows bit for bit, and with k = -1 (folds set or not) so are the first three sums; sum_held dev +
    sum_train dev of the fold is sum_train dev of k = -1 within the summation error (n + 64) 2^-53 sum dev; a held-out row
    stays at weight 0 through two rounds of solve and step."""
    _reaches(n, cap, branch)
    X, y, o, x = _row_case(n)
    wmin, emax, K, k = 1e-3, 7.0, 3, 1
    ids = (np.arange(n) % K).astype(np.int32)
    held = ids == k
    fa, fb = _loss(monkeypatch, y, X, o, cap), _loss(monkeypatch, y, X, o, cap)
    fa.set_folds(ids, K)
    for g in (fa, fb):
        cd.initialize_(g, x)
    eta = fa.y - fa.r
    dev_t, cap_t = PN.rows(y, eta, o, wmin, emax)[4], PN.rows(y, eta, o, wmin, emax)[6]
    plain = _step(fb, -1, 0, wmin, emax)                     # no folds were ever set
    assert np.array_equal(_step(fa, -1, 0, wmin, emax), plain)
    ro = _step(fa, k, 0, wmin, emax)
    out = _step(fa, k, 1, wmin, emax)
    assert np.array_equal(ro, out)
    assert np.array_equal(_step(fb, -1, 1, wmin, emax), plain)
    w, z, r = fa.w, fa.y, fa.r
    np.testing.assert_array_equal(w[held], np.zeros(held.sum()))
    np.testing.assert_array_equal(r[held], np.zeros(held.sum()))
    np.testing.assert_array_equal(z[held], eta[held])
    for u, v in ((w, fb.w), (z, fb.y), (r, fb.r)):
        np.testing.assert_array_equal(u[~held], v[~held])
    assert out[3] == plain[3] == cap_t.sum()                 # capped counts the live rows, held out or not
    assert out[2] == (fb.w[~held] == wmin).sum()
    split = abs((out[4] + out[5]) - plain[5])
    print(f"poisson fold step n={n} cap={cap}: held {int(held.sum())}, |held + train - all| dev {split / (U * plain[5]):.2f} ulp")
    assert split <= (n + 64) * U * plain[5]
    assert abs(out[4] - dev_t[held].sum()) <= (n + 64) * U * (y + np.exp(np.minimum(eta + o, emax)))[held].sum()
    sw, _ = _wmoments(fa)
    assert abs(sw - w.sum()) <= n * U * w.sum()              # pads zero
    # two rounds of solve and step: the held-out rows keep weight 0 and their eta_lin follows the iterate
    xs = x                                                   # (warm: the iterate the handle holds)
    cd.check(fa._L.cdh_set_reuse_residual(fa._h, 1), fa._h)
    for _ in range(2):
        cd.coordinateDescent_(xs, fa, cd.ProxL1(0.01), cd.CDOptions(maxIter=200, optTol=1e-10, randomize=False))
        _step(fa, k, 1, wmin, emax)
        np.testing.assert_array_equal(fa.w[held], np.zeros(held.sum()))
        np.testing.assert_array_equal(fa.r[held], np.zeros(held.sum()))
        np.testing.assert_allclose(fa.y[held], (X @ xs.dense())[held], rtol=0, atol=1e-12)
        assert np.all(fa.w[~held] >= wmin)
    fa.close()
    fb.close()


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


def _big_case():
    X, y, o, _ = PN.make_data(3, 3000, 400, 10)
    return X, y, o, PN.lambda_max(X, y, o)


def test_read_only_step_leaves_a_cache_served_path_as_it_was():
    X, y, o, lmax = _big_case()
    opts = cd.CDOptions(maxIter=500, optTol=1e-12, randomize=False)
    f = cd.CDPoissonLoss(y, X, o)
    f.irls_step(True)                                        # one round's weighted lasso, solved along a path from the cache
    f.set_gradient_cache(2)
    cd.check(f._L.cdh_set_reuse_residual(f._h, 1), f._h)
    x = cd.SparseIterate(400)
    for frac in (0.8, 0.6, 0.45, 0.3):
        cd.coordinateDescent_(x, f, cd.ProxL1(frac * lmax), opts)
    assert f.cache_stats()["passes"] > 0 and x.nnz > 0                         # the cache is serving
    # the catch-up is cdh_loadings': a pending residual is brought up to date, and nothing else moves
    before = _snapshot(f)
    a = _step(f, -1, 0)
    after = _snapshot(f)
    _same(before, after, but=("residual_catchups",))
    assert 0 <= after["cache"]["residual_catchups"] - before["cache"]["residual_catchups"] <= 1
    # ... and with r up to date, nothing at all: twice the same bits, every counter, and r itself
    r0 = f.r
    before = _snapshot(f)
    b, c = _step(f, -1, 0), _step(f, -1, 0)
    after = _snapshot(f)
    assert np.array_equal(a, b) and np.array_equal(b, c)
    _same(before, after)
    np.testing.assert_array_equal(f.r, r0)
    rows = PN.rows(y, X @ x.dense(), o)
    assert abs(b[0] - rows[3].sum()) <= 1e-12 * np.abs(rows[3]).sum()           # F's own nll at the iterate, whatever z and w are
    assert abs(b[5] - rows[4].sum()) <= 1e-12 * rows[4].sum()
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
    X, y, o, _ = PN.make_data(3, n, p, 5)
    lam = 0.1 * PN.lambda_max(X, y, o)
    opts = cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)
    want = PN.poisson_lasso(X, y, o, lam, maxIter=3, optTol=0.0)[0]
    assert np.count_nonzero(want) >= 3
    got = {}
    for kind, env in KINDS.items():
        with monkeypatch.context() as m:                     # read when the handle is made; the suite's own setting comes back
            for k, v in env.items():
                m.setenv(k, v)
            f = cd.CDPoissonLoss(y, X, o)
        x = cd.SparseIterate(p)
        sol = cd.poissonLasso_(x, f, cd.ProxL1(lam), opts, cd.IRLSOptions(maxIter=3, optTol=0.0))
        assert sol.rounds == 3 and not sol.converged and sol.monotone and sol.capped == 0
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


# ---- solves --------------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(seed):
    """The twin's answers for a data set, computed once: one solve at 0.1 lambda_max and the standardised path at PN.FRACS."""
    if seed not in _REF:
        X, y, o, _ = PN.make_data(seed)
        icpt = PN.DATASETS[seed][3]
        lmax = PN.lambda_max(X, y, o, intercept=icpt)
        one = PN.poisson_lasso(X, y, o, 0.1 * lmax, optTol=1e-10, intercept=icpt)
        sx = np.sqrt((X * X).sum(axis=0) / X.shape[0])
        lmax_s = PN.lambda_max(X, y, o, sx, intercept=icpt)
        path = PN.poisson_path(X, y, o, np.array(PN.FRACS) * lmax_s, True, optTol=1e-10, intercept=icpt)
        _REF[seed] = (X, y, o, icpt, lmax, one, sx, lmax_s, path)
    return _REF[seed]


def _kkt_ok(X, f_counts, f_offset, beta, lam, omega, b0, icpt):
    """The KKT conditions of F from the handle's own counts and offset and a host X: nothing of the twin."""
    n, p = X.shape
    om = np.ones(p) if omega is None else omega
    res = f_counts - np.exp(X @ beta + b0 + f_offset)
    g = X.T @ res / n
    nz = beta != 0.0
    on = float(np.max(np.abs(g[nz] - lam * om[nz] * np.sign(beta[nz])))) if nz.any() else 0.0
    off = float(np.max(np.abs(g[~nz]) - lam * om[~nz])) if (~nz).any() else -np.inf
    ic = float(abs(np.sum(res)) / n) if icpt else 0.0
    assert on <= 1e-8 and off <= 1e-8 and ic <= 1e-8, (on, off, ic)
    return max(on, off, ic)


@pytest.mark.parametrize("seed", sorted(PN.DATASETS))
def test_solves_against_the_twin_and_the_kkt_conditions(seed):
    """poissonLasso, poissonLambdaMax and PoissonLassoPath (lambda / lambda_max in PN.FRACS, standardised) on the data sets of
    tests/test_poisson_host.py; inner optTol 1e-12, IRLS optTol 1e-10.  The rounds equal the twin's; beta against the twin
    at the binomial solve test's 1e-10 (measured on an MI355X: LAB_NOTES "Poisson lasso"); the KKT conditions of F at 1e-8
    from f.counts, f.offset and the host's X, whatever the twin says; F never rising."""
    X, y, o, icpt, lmax, one, sx, lmax_s, path = _reference(seed)
    n, p = X.shape
    opts = cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)
    irls = cd.IRLSOptions(optTol=1e-10)
    X1 = PN.with_ones(X) if icpt else X
    f = cd.CDPoissonLoss(y, X1, o)
    counts, offset = f.counts, f.offset
    # lambda_max from the device, with the offset (and the intercept): at 1.0001 of it nothing enters, at 0.999 something does
    got = cd.poissonLambdaMax(f, fit_intercept=icpt)
    print(f"lambda_max [seed {seed}]: device {got:.15g} twin {lmax:.15g} rel {abs(got - lmax) / lmax:.1e}")
    assert abs(got - lmax) <= 1e-12 * lmax
    assert abs(cd.poissonLambdaMax(f, np.r_[sx, 1.0][: f.p], fit_intercept=icpt) - lmax_s) <= 1e-12 * lmax_s
    f.close()
    above = cd.poissonLasso(X, y, 1.0001 * lmax, options=opts, irls=irls, fit_intercept=icpt, offset=o)
    below = cd.poissonLasso(X, y, 0.999 * lmax, options=opts, irls=irls, fit_intercept=icpt, offset=o)
    assert above.x.nnz == 0 and below.x.nnz >= 1 and above.converged and below.converged
    # the front end from a matrix
    worst = 0.0
    sol = cd.poissonLasso(X, y, 0.1 * lmax, options=opts, irls=irls, fit_intercept=icpt, offset=o)
    assert len(sol.x) == p and sol.converged and sol.monotone and sol.capped == 0 and (sol.intercept is not None) == icpt
    assert sol.rounds == one[2], (sol.rounds, one[2])
    worst = max(worst, float(np.max(np.abs(sol.x.dense() - one[0]))), abs((sol.intercept or 0.0) - one[1]))
    _kkt_ok(X, counts, offset, sol.x.dense(), 0.1 * lmax, None, sol.intercept or 0.0, icpt)
    assert abs(sol.nll - PN.objective(X, y, o, sol.x.dense(), 0.0, None, sol.intercept or 0.0)) <= 1e-12
    dev_t = PN.deviance(y, X @ sol.x.dense() + (sol.intercept or 0.0), o).sum()
    assert abs(sol.deviance - dev_t) <= 1e-10 * dev_t
    # the path
    lams = np.array(PN.FRACS) * lmax_s
    res = cd.PoissonLassoPath(X, y, lams, opts, irls, fit_intercept=icpt, offset=o)
    assert len(res.betapath) == 5 and len(res.nll) == 5 and len(res.deviance) == 5 and all(res.converged)
    assert res.rounds == [t[2] for t in path], (res.rounds, [t[2] for t in path])
    assert res.betapath[0].nnz >= 1 and res.betapath[-1].nnz > res.betapath[0].nnz
    for lam, b, bi, t in zip(lams, res.betapath, res.intercepts, path):
        assert len(b) == p
        worst = max(worst, float(np.max(np.abs(b.dense() - t[0]))), abs((bi or 0.0) - t[1]))
        _kkt_ok(X, counts, offset, b.dense(), lam, sx, bi or 0.0, icpt)
    print(f"solves [seed {seed}]: max|beta_gpu - beta_twin| {worst:.2e}, rounds {sol.rounds}, path rounds {res.rounds}")
    assert worst <= 1e-10, worst


# ---- cross-validation ------------------------------------------------------------------------------------------------------------
def _cv_data():
    X, y, o, _ = PN.make_data(5, 240, 12, 4)
    return X, y, o


_CV = {}


def _cv_twin(K, icpt, std):
    if (K, icpt, std) not in _CV:
        X, y, o = _cv_data()
        sx = np.sqrt((X * X).sum(axis=0) / 240) if std else None
        lams = np.geomspace(0.8, 0.03, 6) * PN.lambda_max(X, y, o, sx, intercept=icpt)
        ids = CV.fold_ids(240, K, 0)
        _CV[(K, icpt, std)] = (lams, ids, PN.cv(X, y, o, lams, K, ids, icpt, std))
    return _CV[(K, icpt, std)]


def _opts():
    return cd.CDOptions(maxIter=10000, optTol=1e-12, randomize=False)


@pytest.mark.parametrize("K,icpt,std", [(3, True, True), (4, False, True), (4, True, False), (3, False, False)],
                         ids=["K3-b-std", "K4-std", "K4-b-raw", "K3-raw"])
def test_cv_poisson_path_against_the_twin(K, icpt, std):
    """n = 240, p = 12, with an offset, 6 lambda from 0.8 to 0.03 of lambda_max; inner optTol 1e-12, IRLS optTol 1e-10.  Every
    coefficient of every fold's path within 1e-10 of the twin's fit on the training rows ALONE, the deviances within 1e-9
    relative (the binomial cross-validation's figures; measured: LAB_NOTES "Poisson lasso"), the selections equal, `path`
    bit for bit PoissonLassoPath on a fresh handle."""
    X, y, o = _cv_data()
    lams, ids, t = _cv_twin(K, icpt, std)
    p, m = X.shape[1], len(lams)
    irls = cd.IRLSOptions(optTol=1e-10)
    res = cd.cvPoissonLassoPath(X, y, lams, K=K, options=_opts(), irls=irls, standardizeX=std, fit_intercept=icpt, offset=o,
                                keep_fold_paths=True)
    assert isinstance(res, cd.CVPoissonLassoPathResult) and res.measure == "deviance"
    np.testing.assert_array_equal(res.fold_sizes, t["sizes"])
    np.testing.assert_array_equal(res.lambdapath, lams)
    assert res.fold_deviance.shape == res.train_deviance.shape == res.rounds.shape == res.converged.shape == (K, m)
    assert res.converged.all() and res.rounds.max() <= 12 and res.rounds.min() >= 1
    worst = 0.0
    for k in range(K):
        fp = res.fold_paths[k]
        assert len(fp.betapath) == m and fp.rounds == res.rounds[k].tolist()
        assert fp.rounds == [s[2] for s in t["paths"][k]]
        for b, bi, s in zip(fp.betapath, fp.intercepts, t["paths"][k]):
            assert len(b) == p and (bi is not None) == icpt
            worst = max(worst, float(np.max(np.abs(b.dense() - s[0]))), abs((bi or 0.0) - s[1]))
    edev = float(np.max(np.abs(res.fold_deviance - t["fold_deviance"]) / t["fold_deviance"]))
    etdev = float(np.max(np.abs(res.train_deviance - t["train_deviance"]) / t["train_deviance"]))
    print(f"cv poisson path [K={K} intercept={icpt} standardize={std}]: max|beta_gpu - beta_twin| {worst:.2e}, deviance rel "
          f"{edev:.2e} (held out) {etdev:.2e} (training), index_min {res.index_min} index_1se {res.index_1se}, "
          f"rounds {int(res.rounds.sum())}")
    assert worst <= 1e-10, worst
    assert edev <= 1e-9 and etdev <= 1e-9
    assert (res.index_min, res.index_1se) == (t["index_min"], t["index_1se"]) and 0 < res.index_min
    assert res.lambda_min == lams[res.index_min] and res.lambda_1se == lams[res.index_1se]
    np.testing.assert_allclose(res.cvm, t["cvm"], rtol=1e-9)
    np.testing.assert_allclose(res.cvsd, t["cvsd"], rtol=1e-6)
    # the path on all rows is what PoissonLassoPath makes of a fresh handle, bit for bit
    ref = cd.PoissonLassoPath(X, y, lams, _opts(), irls, standardizeX=std, fit_intercept=icpt, offset=o)
    assert res.path.rounds == ref.rounds and res.path.intercepts == ref.intercepts and res.path.nll == ref.nll
    assert res.path.deviance == ref.deviance
    for a, b in zip(res.path.betapath, ref.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())
        assert a.nzval2ind.tolist() == b.nzval2ind.tolist()


def test_a_loss_that_was_passed_in_comes_back_without_folds():
    X, y, o = _cv_data()
    lams, ids, t = _cv_twin(4, False, True)
    f = cd.CDPoissonLoss(y, X, o)
    mode = f.gradient_cache_mode()
    res = cd.cvPoissonLassoPath(f, None, lams, K=4, options=_opts(), irls=cd.IRLSOptions(optTol=1e-10))
    assert (res.index_min, res.index_1se) == (t["index_min"], t["index_1se"]) and f.gradient_cache_mode() == mode
    # the handle's weights are what a plain step writes -- no zeros: the path on all rows ran last -- and the folds are gone
    assert np.all(f.w > 0) and len(res.path.betapath) == len(lams)
    last = res.path.betapath[-1].dense()
    np.testing.assert_allclose(f.w, PN.rows(y, X @ last, o)[0], rtol=1e-6)
    out = np.zeros(6)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    assert f._L.cdh_glm_poisson_irls(f._h, 0, 0, 1e-5, 50.0, po) == BAD
    assert b"cdh_set_folds" in f._L.cdh_last_error(f._h)
    # a fold that raises (the rounds of IRLS refuse cold starts) drops the folds too
    with pytest.raises(cd.ArgumentError, match="warmStart"):
        cd.cvPoissonLassoPath(f, None, lams, K=4, options=cd.CDOptions(warmStart=False))
    assert f._L.cdh_glm_poisson_irls(f._h, 0, 0, 1e-5, 50.0, po) == BAD
    assert b"cdh_set_folds" in f._L.cdh_last_error(f._h)
    assert f._L.cdh_glm_poisson_irls(f._h, -1, 0, 1e-5, 50.0, po) == OK
    f.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    rng = np.random.default_rng(4)
    n, p, K = 50, 4, 3
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = rng.poisson(1.5, n).astype(np.float64)
    o = rng.uniform(-0.5, 0.5, n)
    L = cd._lib.lib()
    out6 = np.zeros(6)
    po = out6.ctypes.data_as(C.POINTER(C.c_double))

    def refused(h, status, word=None):
        assert status == BAD and len(L.cdh_last_error(h)) > 0, (status, L.cdh_last_error(h))
        assert word is None or word in L.cdh_last_error(h), (word, L.cdh_last_error(h))

    f = cd.CDPoissonLoss(y, X, o)
    x = cd.SparseIterate(p)
    x[2] = 0.5
    cd.initialize_(f, x)
    for apply in (0, 1):                                                       # k >= 0 without folds
        refused(f._h, L.cdh_glm_poisson_irls(f._h, 0, apply, 1e-5, 50.0, po), b"needs cdh_set_folds first")
    f.set_folds(np.arange(n) % K, K)
    _step(f, 1, 1)
    state = lambda: (f.counts, f.offset, f.y, f.r, f.w, _step(f, 1, 0))       # noqa: E731
    before = state()
    assert np.count_nonzero(f.w == 0.0) == np.count_nonzero(np.arange(n) % K == 1)
    # counts and offsets that are refused, the message naming the row
    for bad in (-0.1, -1.0, np.nan, np.inf, -np.inf):
        cnt = y.copy()
        cnt[17] = bad
        refused(f._h, L.cdh_glm_set_counts(f._h, _vp(cnt), _vp(o)), b"counts[17]")
    for bad in (np.nan, np.inf, -np.inf):
        off = o.copy()
        off[23] = bad
        refused(f._h, L.cdh_glm_set_counts(f._h, _vp(y), _vp(off)), b"offset[23]")
    refused(f._h, L.cdh_glm_set_counts(f._h, None, _vp(o)))
    refused(f._h, L.cdh_glm_get_offset(f._h, None))
    refused(f._h, L.cdh_glm_get_labels(f._h, None))
    # the step's own arguments
    for apply in (0, 1):
        refused(f._h, L.cdh_glm_poisson_irls(f._h, -2, apply, 1e-5, 50.0, po), b"k must be a fold")
        refused(f._h, L.cdh_glm_poisson_irls(f._h, K, apply, 1e-5, 50.0, po), b"below the K")
        refused(f._h, L.cdh_glm_poisson_irls(f._h, 255, apply, 1e-5, 50.0, po), b"below the K")
        for wmin in (0.0, -1e-5, np.nan, np.inf):
            refused(f._h, L.cdh_glm_poisson_irls(f._h, 1, apply, wmin, 50.0, po), b"wmin")
        for emax in (0.0, -1.0, 700.5, np.nan, np.inf):
            refused(f._h, L.cdh_glm_poisson_irls(f._h, 1, apply, 1e-5, emax, po), b"eta_max")
        refused(f._h, L.cdh_glm_poisson_irls(f._h, 1, apply, 1e-5, 50.0, None))
    for apply in (2, -1):
        refused(f._h, L.cdh_glm_poisson_irls(f._h, 1, apply, 1e-5, 50.0, po), b"apply")
    # the binomial step on a Poisson handle
    for apply in (0, 1):
        refused(f._h, L.cdh_glm_irls(f._h, apply, 1e-5, po), b"Poisson")
        refused(f._h, L.cdh_glm_irls_fold(f._h, 1, apply, 1e-5, po), b"Poisson")
    # an exchange installed makes the handle a row shard: refused, and accepted again when it is gone
    f.set_host_exchange(lambda buf: None, 0, 1)
    for apply in (0, 1):
        refused(f._h, L.cdh_glm_poisson_irls(f._h, 1, apply, 1e-5, 50.0, po), b"row-sharded")
    refused(f._h, L.cdh_glm_set_counts(f._h, _vp(y), None), b"row-sharded")
    f.set_host_exchange(None, 0, 1)
    for a, b in zip(before, state()):
        np.testing.assert_array_equal(a, b)
    assert L.cdh_glm_poisson_irls(f._h, K - 1, 0, 1e300, 700.0, po) == OK      # the last fold, the largest eta_max allowed
    # wmin = 0.3 is the Poisson step's to take (weights are unbounded above), and still refused by the binomial one
    assert L.cdh_glm_poisson_irls(f._h, 1, 0, 0.3, 50.0, po) == OK
    # labels turn the handle binomial again and drop the offset: the Poisson step and the offset are refused
    lab = (y > 1).astype(np.float64)
    cd.check(L.cdh_glm_set_labels(f._h, 0, _vp(lab)), f._h)
    refused(f._h, L.cdh_glm_poisson_irls(f._h, -1, 0, 1e-5, 50.0, po), b"cdh_glm_set_counts")
    refused(f._h, L.cdh_glm_get_offset(f._h, _vp(out6)), b"cdh_glm_set_counts")
    assert L.cdh_glm_irls(f._h, 0, 1e-5, po) == OK
    refused(f._h, L.cdh_glm_irls(f._h, 0, 0.3, po), b"wmin")
    refused(f._h, L.cdh_glm_set_labels(f._h, 1, _vp(lab)), b"family")
    # ... and counts without an offset afterwards find none
    cd.check(L.cdh_glm_set_counts(f._h, _vp(y), None), f._h)
    np.testing.assert_array_equal(f.offset, np.zeros(n))
    # a least-squares handle: refused, with counts and folds still in it
    cd.check(L.cdh_set_loss(f._h, cd._lib.CDH_LS), f._h)
    refused(f._h, L.cdh_glm_poisson_irls(f._h, 1, 0, 1e-5, 50.0, po), b"CDH_WLS")
    refused(f._h, L.cdh_glm_set_counts(f._h, _vp(y), None), b"CDH_WLS")
    f.close()
    # a binomial handle from the start
    b = cd.CDLogisticLoss(lab, X)
    for apply in (0, 1):
        refused(b._h, L.cdh_glm_poisson_irls(b._h, -1, apply, 1e-5, 50.0, po), b"cdh_glm_set_counts")
    np.testing.assert_array_equal(b.labels, lab)
    b.close()
    # NULL handles
    for status in (L.cdh_glm_set_counts(None, _vp(y), None), L.cdh_glm_get_offset(None, _vp(y)),
                   L.cdh_glm_poisson_irls(None, -1, 0, 1e-5, 50.0, po)):
        assert status == BAD
    # a weighted handle without counts
    g = cd.CDWeightedLSLoss(y, X, np.ones(n))
    refused(g._h, L.cdh_glm_poisson_irls(g._h, -1, 1, 1e-5, 50.0, po), b"cdh_glm_set_counts")
    refused(g._h, L.cdh_glm_get_offset(g._h, _vp(out6)), b"cdh_glm_set_counts")
    np.testing.assert_array_equal(g.y, y)
    np.testing.assert_array_equal(g.w, np.ones(n))
    g.close()
    # not CDH_WLS
    ls = cd.CDLeastSquaresLoss(y, X)
    refused(ls._h, L.cdh_glm_set_counts(ls._h, _vp(y), _vp(o)), b"CDH_WLS")
    np.testing.assert_array_equal(ls.y, y)
    np.testing.assert_array_equal(ls.r, y)
    ls.close()
    # fp32 storage, and a row shard: refused, and still working handles
    y32 = y.astype(np.float32)
    for dtype, n_total, yy in ((cd._lib.CDH_F32, n, y32), (cd._lib.CDH_F64, 2 * n, y)):
        h = C.c_void_p()
        assert L.cdh_create(C.byref(h), dtype, cd._lib.CDH_WLS, n, n_total, 0, p, 0) == OK
        assert L.cdh_set_y(h, _vp(yy)) == OK
        refused(h, L.cdh_glm_set_counts(h, _vp(y), _vp(o)))
        refused(h, L.cdh_glm_poisson_irls(h, -1, 0, 1e-5, 50.0, po))
        back = np.zeros_like(yy)
        assert L.cdh_get_y(h, _vp(back)) == OK and np.array_equal(back, yy)
        assert L.cdh_destroy(h) == OK
