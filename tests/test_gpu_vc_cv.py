"""Leave-one-out bandwidth selection on the device: cdh_vc_set_point_loo (k_vc_weights with a left-out row, k_vc_expand<LOO>),
cdh_resid_wmoments (k_resid_moments<T, true>), cdh_get_X_row (k_gather_row) and lvocv_locpolyl1 on top of them, held to the numpy
restatement in tests/_vc_cv_numpy.py (pinned against closed forms in tests/test_vc_cv_host.py) and to `oracle`'s
CDWeightedLSLoss and driver."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
from _vc_numpy import expand, gen_data, oracle_locpolyl1
from _vc_cv_numpy import SIGMA_TOL, oracle_lvocv

pytestmark = pytest.mark.gpu

KERNELS = {"gaussian": cd.GaussianKernel, "epanechnikov": cd.EpanechnikovKernel}
NV = {np.dtype(np.float64): 2, np.dtype(np.float32): 4}         # elements per 16-byte vector


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _rows(n, dtype):
    """first, last, the first element of the last (partial) vector, and an odd row in the middle of a row chunk"""
    nv = NV[np.dtype(dtype)]
    return sorted({0, n - 1, (n - 1) // nv * nv, n // 2 + 1})


# ---- 1. the leave-one-out point ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 1237, 300_000])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_leave_one_out_setup(dtype, n):
    """w[row] == 0 and every other weight is the bit set_point(kernel, z[row]) writes; the expansion is the recurrence, bit
    for bit; stdX is cdh_col_wrms of the state left behind, bit for bit (same sums, same order); the scores against a long
    double sum of the same stored values: each is a sum of n products accumulated in double by fma, so any order of
    summation is within n 2^-53 sum_i |w_i x_ij y_i| (the argument of tests/test_gpu_kernel_sums.py)."""
    rng = np.random.default_rng(n)
    pb = 3
    X = np.asfortranarray(rng.standard_normal((n, pb)).astype(dtype))
    z, y = rng.random(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    worst = 0.0
    for degree in range(4):
        ep = pb * (degree + 1)
        f = cd.CDVaryingCoefficientLoss(y, X, z, degree)
        for kind, h in (("gaussian", 0.1), ("epanechnikov", 0.25)):
            kern = KERNELS[kind](h)
            for row in _rows(n, dtype):
                std, scores = f.set_point_leave_out(kern, row)
                w, got = f.w, f.X_cols(0, ep)
                assert np.array_equal(std, cd.stdX(f, weighted=True)), (degree, kind, row)
                f.set_point(kern, float(z[row]))
                w_ref = f.w
                assert w[row] == 0 and w_ref[row] > 0, (degree, kind, row)
                keep = np.arange(n) != row
                assert np.array_equal(w[keep], w_ref[keep]), (degree, kind, row)
                eX = expand(X, z, z[row], degree)
                assert np.array_equal(got, eX), (degree, kind, row)
                wy = w.astype(np.longdouble) * y.astype(np.longdouble)
                terms = eX.astype(np.longdouble) * wy[:, None]
                want = np.abs(terms.sum(axis=0)).astype(np.float64)
                bound = (n * 2.0 ** -53 * np.abs(terms).sum(axis=0)).astype(np.float64)
                assert np.all(np.abs(scores - want) <= bound), (degree, kind, row, scores - want, bound)
                worst = max(worst, float(np.max(np.abs(scores - want) / bound)))
        f.close()
    print(f"loo setup n={n} {np.dtype(dtype).name}: worst score error {worst:.3e} of its bound")


@pytest.mark.parametrize("n", [33, 1237, 300_000])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_scores_and_scales_are_exact_on_small_integer_data(dtype, n):
    """Epanechnikov with h = 1 on z in {0, 1/4, .., 1}: d = z - z0 = k / 4, w = 0.75 (1 - d^2) = 3 (16 - k^2) / 64, the
    powers d^l = k^l / 4^l, |x| <= 127, |y| <= 511 integers -- every weight, every expanded entry (at most 12 significant
    bits: fp32 holds them), every product w v y (a multiple of 2^-12 below 2^16) and every partial sum over 300 000 rows
    (below 2^35) is representable, so the sums equal numpy's to the bit whatever the order; likewise sum w v^2 (multiples of
    2^-18, below 2^37)."""
    rng = np.random.default_rng(n + 1)
    pb = 5
    X = np.asfortranarray(rng.integers(-127, 128, size=(n, pb)).astype(dtype))
    z = (rng.integers(0, 5, size=n) / 4.0).astype(dtype)
    y = rng.integers(-511, 512, size=n).astype(dtype)
    kern = cd.EpanechnikovKernel(1.0)
    for degree in range(4):
        f = cd.CDVaryingCoefficientLoss(y, X, z, degree)
        for row in _rows(n, dtype):
            std, scores = f.set_point_leave_out(kern, row)
            d = z.astype(np.float64) - float(z[row])
            w = np.where(np.abs(d) >= 1.0, 0.0, 0.75 * (1.0 - d * d))
            w[row] = 0.0
            assert np.array_equal(f.w.astype(np.float64), w)
            eX = expand(X, z, z[row], degree).astype(np.float64)
            assert np.array_equal(scores, np.abs((eX * (w * y.astype(np.float64))[:, None]).sum(axis=0))), (degree, row)
            assert np.array_equal(std, np.sqrt((eX * eX * w[:, None]).sum(axis=0) / n)), (degree, row)
        f.close()


@pytest.mark.parametrize("pb,degree", [(1366, 2), (2049, 1)])
@pytest.mark.parametrize("n", [33, 5003])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_point_is_exact_across_the_column_batch_boundary(dtype, n, pb, degree):
    """p = 4098 expanded columns: two k_vc_expand launches, over columns [0, 4096) and [4096, 4098).  At degree 2 the group
    of the last base column, columns 4095 .. 4097, straddles the boundary: both launches expand it (the same values written
    twice) and each keeps the sums of its own columns; at degree 1 the boundary falls between two groups.  n = 33 has pad
    rows and one row chunk; at n = 5003 the two launches split their rows into different numbers of chunks.  The data of
    test_scores_and_scales_are_exact_on_small_integer_data (z0 = 1/2 is a quarter too), so every sum equals numpy's to the
    bit whatever the order: for set_point and for the leave-one-out point at the first and the last row, the expanded design
    is the recurrence, the scales are the numpy sums and cdh_col_wrms of the state left behind, the scores the numpy sums."""
    rng = np.random.default_rng(n + pb)
    p = pb * (degree + 1)
    assert p == 4098
    X = np.asfortranarray(rng.integers(-127, 128, size=(n, pb)).astype(dtype))
    z = (rng.integers(0, 5, size=n) / 4.0).astype(dtype)
    y = rng.integers(-511, 512, size=n).astype(dtype)
    kern = cd.EpanechnikovKernel(1.0)
    f = cd.CDVaryingCoefficientLoss(y, X, z, degree)
    for row in (None, 0, n - 1):
        z0 = 0.5 if row is None else float(z[row])
        std, scores = (f.set_point(kern, z0), None) if row is None else f.set_point_leave_out(kern, row)
        d = z.astype(np.float64) - z0
        w = np.where(np.abs(d) >= 1.0, 0.0, 0.75 * (1.0 - d * d))
        if row is not None:
            w[row] = 0.0
        assert np.array_equal(f.w.astype(np.float64), w), row
        eX = expand(X, z, z0, degree)
        assert np.array_equal(f.X_cols(0, p), eX), row
        eX = eX.astype(np.float64)
        assert np.array_equal(std, np.sqrt((eX * eX * w[:, None]).sum(axis=0) / n)), row
        assert np.array_equal(std, cd.stdX(f, weighted=True)), row
        if row is not None:
            assert np.array_equal(scores, np.abs((eX * (w * y.astype(np.float64))[:, None]).sum(axis=0))), row
    f.close()


# ---- 2. cdh_resid_wmoments --------------------------------------------------------------------------------------------
def _wmoments(f):
    sw, swr2 = C.c_double(), C.c_double()
    cd.check(f._L.cdh_resid_wmoments(f._h, C.byref(sw), C.byref(swr2)), f._h)
    return sw.value, swr2.value


@pytest.mark.parametrize("n", [33, 5003, 300_000])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_resid_wmoments_is_exact_on_summable_integers(dtype, n):
    """|x| <= 7, |y| <= 100, three integer coefficients of at most 3: |r| <= 163 and w <= 3 are integers, sum w r^2 < 2^35."""
    rng = np.random.default_rng(n)
    p = 6
    X = np.asfortranarray(rng.integers(-7, 8, size=(n, p)).astype(dtype))
    y = rng.integers(-100, 101, size=n).astype(dtype)
    w = rng.integers(0, 4, size=n).astype(dtype)
    f = cd.CDWeightedLSLoss(y, X, w)
    x = cd.SparseIterate(p)
    x[2], x[5], x[6] = 3.0, -2.0, 1.0
    cd.initialize_(f, x)
    r = y.astype(np.float64) - X.astype(np.float64) @ x.dense()
    assert np.array_equal(f.r.astype(np.float64), r)
    w64 = w.astype(np.float64)
    assert _wmoments(f) == (float(w64.sum()), float((w64 * r * r).sum()))
    assert cd.getSigma(f) == float(np.sqrt((w64 * r * r).sum() / w64.sum()))
    f.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_resid_wmoments_agrees_with_the_weighted_gram_block(dtype):
    """sum w r^2 and cdh_gram_weighted's *out_q sum the same n non-negative terms in double: each is within n 2^-53 of the
    exact sum, relative."""
    (X, z, y) = gen_data(np.random.default_rng(8), 5003, 3, 4, dtype)
    f = cd.CDVaryingCoefficientLoss(y, X, z, 1)
    f.set_point_leave_out(cd.GaussianKernel(0.2), 77)
    idx1 = np.arange(1, 5, dtype=np.int64)
    G, c, q = np.zeros((4, 4)), np.zeros(4), C.c_double()
    cd.check(f._L.cdh_gram_weighted(f._h, 4, _vp(idx1), _vp(G), _vp(c), C.byref(q)), f._h)
    sw, swr2 = _wmoments(f)
    print(f"wmoments {np.dtype(dtype).name}: sum w r^2 {swr2!r} gram q {q.value!r}")
    assert abs(swr2 - q.value) <= 2 * 5003 * 2.0 ** -53 * q.value
    w = f.w.astype(np.longdouble)
    assert abs(sw - float(w.sum())) <= 5003 * 2.0 ** -53 * float(w.sum())
    f.close()


@pytest.mark.parametrize("how", ["one-launch", "gradient-cache"])
def test_resid_wmoments_after_a_solve_that_left_the_residual_behind(how):
    """The one-launch solve leaves r unformed (lazy), covariance-form visits leave it owing moves: the moments must be those
    of y - X beta all the same.  Asked BEFORE anything else reads r; then f.r (which the call has brought up to date) gives
    the reference sums in long double."""
    (X, z, y) = gen_data(np.random.default_rng(9), 2000, 3, 20)
    w = np.random.default_rng(10).random(2000) + 0.5
    f = cd.CDWeightedLSLoss(y, X, w)
    if how == "one-launch":
        f.set_onchip_solve(True)
    else:
        f.set_gradient_cache(3)
    x = cd.SparseIterate(f.p)
    sx = cd.stdX(f, weighted=True)
    for lam in (0.3, 0.1, 0.05):
        cd.coordinateDescent_(x, f, cd.ProxL1(lam, sx), cd.CDOptions(maxIter=2000, optTol=1e-12, randomize=False))
    if how == "one-launch":
        assert f.onchip_stats()["solves"] >= 3
    else:
        print(f"cache {f.cache_stats()}")
    sw, swr2 = _wmoments(f)
    r = y - X @ x.dense()
    wl, rl = w.astype(np.longdouble), r.astype(np.longdouble)
    want = float((wl * rl * rl).sum())
    # r itself is y - X beta formed in double (nnz fmas per row): relative error of r^2 about 2 (nnz + 1) 2^-53 sum|terms| / |r|
    slack = 4 * (x.nnz + 2) * 2.0 ** -53 * float((wl * (np.abs(y) + np.abs(X) @ np.abs(x.dense())) * np.abs(rl)).sum())
    print(f"wmoments after {how}: {swr2!r} want {want!r} slack {slack:.3e}")
    assert x.nnz > 0 and abs(swr2 - want) <= 2000 * 2.0 ** -53 * want + slack
    assert abs(sw - float(wl.sum())) <= 2000 * 2.0 ** -53 * float(wl.sum())
    assert np.all(np.abs(f.r - r) <= 2 * (x.nnz + 2) * 2.0 ** -53 * (np.abs(y) + np.abs(X) @ np.abs(x.dense())))
    f.close()


# ---- 3. cdh_get_X_row -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 1237])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_get_X_row_is_the_row_of_X_cols(dtype, n):
    rng = np.random.default_rng(n)
    p = 11
    X = np.asfortranarray(rng.standard_normal((n, p)).astype(dtype))
    f = cd.CDLeastSquaresLoss(rng.standard_normal(n).astype(dtype), X)
    full = f.X_cols(0, p)
    for row in (0, n // 2, n - 1):                         # n - 1: the last row before the pad of the leading dimension
        idx1 = np.ascontiguousarray(rng.integers(1, p + 1, size=30), dtype=np.int64)      # repeats, any order, m > p
        out = np.zeros(30)
        cd.check(f._L.cdh_get_X_row(f._h, row, 30, _vp(idx1), _vp(out)), f._h)
        assert np.array_equal(out, full[row, idx1 - 1].astype(np.float64))
    BAD = cd._lib.CDH_BAD_ARG
    one, out = np.array([1], dtype=np.int64), np.zeros(1)
    assert f._L.cdh_get_X_row(f._h, n, 1, _vp(one), _vp(out)) == BAD                   # a pad row is not a row
    assert f._L.cdh_get_X_row(f._h, -1, 1, _vp(one), _vp(out)) == BAD
    assert f._L.cdh_get_X_row(f._h, 0, 0, _vp(one), _vp(out)) == BAD
    assert f._L.cdh_get_X_row(f._h, 0, 1, _vp(np.array([p + 1], dtype=np.int64)), _vp(out)) == BAD
    assert f._L.cdh_get_X_row(f._h, 0, 1, None, _vp(out)) == BAD
    f.close()


# ---- 4. lvocv_locpolyl1 against the yardstick -------------------------------------------------------------------------
OPTS = dict(maxIter=2000, optTol=1e-12, randomize=False)
CASES = {
    "gauss-d1": (gen_data(np.random.default_rng(5), 150, 3, 5), 1, "gaussian", [0.02, 0.1, 0.5], 0.3),
    "epan-d1": (gen_data(np.random.default_rng(6), 150, 3, 5), 1, "epanechnikov", [0.15, 0.3, 0.6], 0.3),
    "gauss-d2": (gen_data(np.random.default_rng(7), 120, 2, 2), 2, "gaussian", [0.05, 0.3], 0.3),
}


def _noisy_data(seed, n):
    """Two columns, one of them carrying 3 (1.5 + sin 4z), under noise of standard deviation 3: sigma is near 3 at every point,
    which is what lets an fp32 run's sigma decisions be told apart from its rounding (test_lvocv_parity_fp32_storage)."""
    rng = np.random.default_rng(seed)
    X, z = rng.standard_normal((n, 2)), rng.random(n)
    y = 3.0 * (1.5 + np.sin(4 * z)) * X[:, 0] + 3.0 * rng.standard_normal(n)
    return np.asfortranarray(X), z, y


ALL_CASES = dict(CASES)
ALL_CASES["noisy-d1"] = (_noisy_data(11, 150), 1, "gaussian", [0.1, 0.4], 0.1)
_yard = {}


def _yardstick(name, dtype=np.float64):
    key = (name, np.dtype(dtype).name)
    if key not in _yard:
        (X, z, y), degree, kind, hArr, lam0 = ALL_CASES[name]
        _yard[key] = oracle_lvocv(O, X.astype(dtype), z.astype(dtype), y.astype(dtype), degree, kind, hArr, lam0, **OPTS)
    return _yard[key]


def _gpu(name, dtype=np.float64, setup=None, opts=OPTS):
    (X, z, y), degree, kind, hArr, lam0 = ALL_CASES[name]
    f = cd.CDVaryingCoefficientLoss(y.astype(dtype), X.astype(dtype), z.astype(dtype), degree)
    if setup:
        setup(f)
    MSE = cd.lvocv_locpolyl1(f, None, None, degree, hArr, KERNELS[kind], lam0, cd.CDOptions(**opts))
    return f, MSE


def _check_against_yardstick(name, f, MSE):
    """The conditions on the inputs first (they are the yardstick's alone), then the device, point by point.
    Refit: the bound of test_refit_solves_the_weighted_normal_equations_on_the_support (tests/test_gpu_varying_coefficient.py),
    4 kappa (|S| + log2 n) 2^-53 |b|_inf.  Prediction: Yh = sum_k x_ik b_k, so a refit within `allowed` moves it by at most
    allowed sum_k |x_ik|, plus the rounding of the dot itself, |S| 2^-53 sum_k |x_ik b_k|: delta_i.  MSE: (Yh + e - y)^2 differs
    from (Yh - y)^2 by at most 2 |Yh - y| |e| + e^2, summed over i; plus the rounding of the n-term sum, n 2^-53 MSE."""
    (X, z, y), degree, kind, hArr, lam0 = CASES[name]
    want_MSE, pts = _yardstick(name)
    n = X.shape[0]
    assert len(pts) == n * len(hArr) == len(f.point_stats)
    assert all(s["converged"] for p in pts for s in p["solves"]) and all(p["S"].any() for p in pts)
    kappa, margin, gap = max(p["kappa"] for p in pts), min(min(p["margins"]) for p in pts), min(p["score_gap"] for p in pts)
    print(f"{name}: yardstick max kappa {kappa:.4g}, min sigma-decision margin {margin:.3e}, min score gap {gap:.3e}")
    assert kappa <= 552 and margin >= 1e-3 and gap >= 1e-5
    bound = np.zeros(len(hArr))
    worst_b = worst_r = 0.0
    for k, (p, d) in enumerate(zip(pts, f.point_stats)):
        at = (name, p["h"], p["row"])
        assert (d["h"], d["row"]) == (p["h"], p["row"])
        assert all(s["converged"] for s in d["solves"]), at
        assert d["sigma_iters"] == p["sigma_iters"], (at, d["sigmas"], p["sigmas"])
        err = float(np.max(np.abs(d["beta"] - p["beta"])))
        worst_b = max(worst_b, err)
        assert err <= 1e-10, (at, err)
        S = cd.get_nonzero_coordinates(d["beta"], X.shape[1], degree, True)
        assert np.array_equal(S, p["S"]), at
        allowed = 4 * p["kappa"] * (S.sum() + np.log2(n)) * 2.0 ** -53 * float(np.max(np.abs(p["refit"])))
        rerr = float(np.max(np.abs(d["refit"] - p["refit"])))
        worst_r = max(worst_r, rerr / allowed)
        assert allowed < 1e-8 and rerr <= allowed, (at, rerr, allowed)
        xs = np.abs(p["xrow"][S])
        delta = allowed * float(xs.sum()) + S.sum() * 2.0 ** -53 * float(xs @ np.abs(p["refit"]))
        assert abs(d["yhat"] - p["yhat"]) <= delta, (at, d["yhat"], p["yhat"], delta)
        bound[k // n] += 2 * abs(p["yhat"] - float(y[p["row"]])) * delta + delta * delta
    bound += n * 2.0 ** -53 * want_MSE
    print(f"{name}: max|dbeta| {worst_b:.3e}; worst refit error {worst_r:.3e} of its bound; MSE gpu {MSE} yardstick {want_MSE} "
          f"|diff| {np.abs(MSE - want_MSE)} bound {bound}")
    assert np.all(np.abs(MSE - want_MSE) <= bound)
    assert int(np.argmin(MSE)) == int(np.argmin(want_MSE))


@pytest.mark.parametrize("name", list(CASES))
def test_lvocv_parity_default_sweep(name):
    f, MSE = _gpu(name, setup=lambda f: f.set_onchip_solve(False))
    assert f.onchip_stats()["solves"] == 0
    _check_against_yardstick(name, f, MSE)
    f.close()


@pytest.mark.parametrize("name", list(CASES))
def test_lvocv_parity_one_launch_solve(name):
    """Every point must see a fresh Gram matrix -- and one only: the solves of its sigma loop share design and weights."""
    f, MSE = _gpu(name, setup=lambda f: f.set_onchip_solve(True))
    st = f.onchip_stats()
    n_points = len(f.point_stats)
    assert st["solves"] >= n_points and st["gram_matrices"] == n_points, st
    _check_against_yardstick(name, f, MSE)
    f.close()


@pytest.mark.parametrize("name", list(CASES))
def test_lvocv_parity_gradient_cache_from_the_first_pass(name):
    f, MSE = _gpu(name, setup=lambda f: f.set_gradient_cache(3))
    print(f"{name}: cache {f.cache_stats()}")
    _check_against_yardstick(name, f, MSE)
    f.close()


@pytest.mark.parametrize("name", ["noisy-d1", "gauss-d1"])
def test_lvocv_parity_fp32_storage(name):
    """fp32 storage against the fp64 yardstick on the fp32-rounded inputs, beta at DESIGN section 2's 3e-4 with the device
    stopping at optTol = 1e-6 (the setting of every fp32 solve in tests/test_gpu_parity.py).

    The sigma-iteration count is asserted where 3e-4 cannot flip a decision.  A beta off by at most e = 3e-4 per
    coefficient moves every residual by at most e L, L = max_i sum_j |X_ij| over the expanded design, hence each sigma --
    a weighted root mean square of residuals -- by at most e L (the screening sigma comes from a fit solved in double on
    sums accumulated in double: its error is of the order 2^-24 |y|, far inside e L); the decision quantity
    q = |s' - s| / s <= 1 then moves by at most (2 e L + q e L) / (s - e L) <= 3 e L / (s_min - e L) =: reach.  A point
    all of whose decisions sit further than reach from 1e-2 is DECIDED: its count must agree.  Wherever the counts agree
    the two sides solved the same last problem and beta is compared; where a decision was free to flip and did, the
    device's last penalty is another sigma's and its beta is nobody's to compare.

    What each case can decide is a property of the inputs, computed on the yardstick alone: a point that stops has a last
    q < 1e-2, so its margin is below 1e-2, and reach is below that only where L / s_min < ~10.  `noisy-d1` (sigma ~ 3,
    L ~ 10) is chosen for that: more than half of its 300 points are decided (243 when this was written), with counts of
    both 1 and 2 among them.  `gauss-d1` (sigma ~ 0.1-0.3) decides none; it stays for beta and for the choice of bandwidth.
    Both must pick the yardstick's bandwidth: the argmin over hArr is identical."""
    dtype, e = np.float32, 3e-4
    (X, z, y), degree, kind, hArr, lam0 = ALL_CASES[name]
    f, MSE = _gpu(name, dtype=dtype, opts=dict(OPTS, optTol=1e-6))
    want_MSE, pts = _yardstick(name, dtype)
    assert all(s["converged"] for p in pts for s in p["solves"])
    X32, z32 = X.astype(dtype), z.astype(dtype)
    decided = []
    for p in pts:
        L = float(np.max(np.abs(expand(X32, z32, z32[p["row"]], degree).astype(np.float64)).sum(axis=1)))
        smin = min(p["sigmas"])
        reach = 3 * e * L / (smin - e * L) if smin > e * L else np.inf
        decided.append(min(p["margins"]) * SIGMA_TOL > reach)
    if name == "noisy-d1":              # the condition on the inputs
        assert sum(decided) > len(pts) // 2 and len({p["sigma_iters"] for p, d in zip(pts, decided) if d}) > 1
    compared, worst = 0, 0.0
    for p, d, dec in zip(pts, f.point_stats, decided):
        at = (name, p["h"], p["row"])
        assert all(s["converged"] for s in d["solves"]), at
        if dec:
            assert d["sigma_iters"] == p["sigma_iters"], (at, d["sigmas"], p["sigmas"])
        if d["sigma_iters"] == p["sigma_iters"]:
            compared += 1
            err = float(np.max(np.abs(d["beta"] - p["beta"])))
            worst = max(worst, err)
            assert err <= e, (at, err)
    print(f"fp32 {name}: {sum(decided)} of {len(pts)} points decided (counts asserted); {compared} with equal counts (beta "
          f"compared, max|dbeta| {worst:.3e}); MSE gpu {MSE} yardstick {want_MSE}")
    assert compared >= max(sum(decided), 1)
    assert int(np.argmin(MSE)) == int(np.argmin(want_MSE))
    f.close()


def test_an_empty_support_predicts_zero_on_the_device():
    """lambda0 so large that every solve ends at beta = 0: no refit, Yh = 0 at every point, MSE[h] = sum(y.^2) -- a sum of
    squares of the stored y, each term exact before the n-term sum."""
    X, z, y = gen_data(np.random.default_rng(1), 30, 2, 1)
    f = cd.CDVaryingCoefficientLoss(y, X, z, 1)
    MSE = cd.lvocv_locpolyl1(f, None, None, 1, [0.1, 0.4], cd.GaussianKernel, 1e3, cd.CDOptions(**OPTS))
    assert len(f.point_stats) == 60
    for d in f.point_stats:
        assert d["refit"] is None and d["yhat"] == 0.0 and not d["beta"].any() and len(d["support"]) == 0
        assert d["sq_err"] == float(y[d["row"]]) ** 2
    acc = 0.0
    for v in y:
        acc += float(v) ** 2
    assert MSE.tolist() == [acc, acc]
    f.close()


def test_lvocv_from_arrays_closes_the_loss_it_builds():
    (X, z, y), degree, kind, hArr, lam0 = CASES["gauss-d2"]
    MSE = cd.lvocv_locpolyl1(X[:40], z[:40], y[:40], degree, [0.3], KERNELS[kind], lam0, cd.CDOptions(**OPTS))
    f = cd.CDVaryingCoefficientLoss(y[:40], X[:40], z[:40], degree)
    assert np.array_equal(MSE, cd.lvocv_locpolyl1(f, None, None, degree, [0.3], KERNELS[kind], lam0, cd.CDOptions(**OPTS)))
    f.close()


# ---- 5. state ---------------------------------------------------------------------------------------------------------
def test_locpolyl1_and_lvocv_on_one_handle_reproduce_fresh_handles():
    (X, z, y), degree, kind, hArr, lam0 = CASES["gauss-d2"]
    zgrid, kern, opt = np.array([0.2, 0.5, 0.8]), KERNELS[kind](0.3), cd.CDOptions(**OPTS)
    fa = cd.CDVaryingCoefficientLoss(y, X, z, degree)
    out_a, outR_a = cd.locpolyl1(fa, None, None, zgrid, degree, kern, 0.05, True, opt)
    fb = cd.CDVaryingCoefficientLoss(y, X, z, degree)
    MSE_b = cd.lvocv_locpolyl1(fb, None, None, degree, [0.3], KERNELS[kind], lam0, opt)
    # locpolyl1 after lvocv_locpolyl1 ...
    out_c, outR_c = cd.locpolyl1(fb, None, None, zgrid, degree, kern, 0.05, True, opt)
    assert np.max(np.abs(out_c - out_a)) <= 1e-10 and np.max(np.abs(outR_c - outR_a)) <= 1e-10
    # ... and the reverse
    n0 = len(fa.point_stats)
    MSE_d = cd.lvocv_locpolyl1(fa, None, None, degree, [0.3], KERNELS[kind], lam0, opt)
    assert np.max(np.abs(MSE_d - MSE_b)) <= 1e-10 * np.max(MSE_b)
    for d, b in zip(fa.point_stats[n0:], fb.point_stats[:X.shape[0]]):
        assert d["sigma_iters"] == b["sigma_iters"] and np.max(np.abs(d["beta"] - b["beta"])) <= 1e-10
    # the expected outcome of the yardstick, for good measure: the fresh handle is the one the parity tests hold to it
    assert np.max(np.abs(out_a - oracle_locpolyl1(O, X, z, y, zgrid, degree, kind, 0.3, 0.05, **OPTS)[0])) <= 1e-10
    fa.close(); fb.close()


# ---- 6. errors --------------------------------------------------------------------------------------------------------
def test_documented_statuses_and_the_handle_stays_usable():
    L = cd._lib.lib()
    BAD, OK = cd._lib.CDH_BAD_ARG, cd._lib.CDH_OK
    n, pb = 200, 3
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.standard_normal((n, pb)))
    z, y = rng.random(n), rng.standard_normal(n)
    std, sc = np.zeros(2 * pb), np.zeros(2 * pb)
    f = cd.CDWeightedLSLoss(y, np.asfortranarray(np.zeros((n, 2 * pb))), np.ones(n))
    assert L.cdh_vc_set_point_loo(f._h, 0, 0.1, 5, _vp(std), _vp(sc)) == BAD              # before cdh_vc_set_data
    assert L.cdh_vc_set_data(f._h, pb, 1, _vp(X), n, _vp(z)) == OK
    assert L.cdh_vc_set_point_loo(f._h, 0, 0.0, 5, _vp(std), _vp(sc)) == BAD              # bandwidth 0
    assert L.cdh_vc_set_point_loo(f._h, 0, -1.0, 5, _vp(std), _vp(sc)) == BAD
    assert L.cdh_vc_set_point_loo(f._h, 7, 0.1, 5, _vp(std), _vp(sc)) == BAD              # unknown kernel
    assert b"kernel" in L.cdh_last_error(f._h)
    assert L.cdh_vc_set_point_loo(f._h, 0, 0.1, n, _vp(std), _vp(sc)) == BAD              # row out of range
    assert L.cdh_vc_set_point_loo(f._h, 0, 0.1, -1, _vp(std), _vp(sc)) == BAD
    assert b"row" in L.cdh_last_error(f._h)
    assert L.cdh_vc_set_point_loo(f._h, 0, 0.1, 5, None, None) == OK                      # either output may be NULL
    assert L.cdh_vc_set_point_loo(f._h, 0, 0.1, 5, None, _vp(sc)) == OK
    assert L.cdh_vc_set_point_loo(f._h, 1, 0.25, n - 1, _vp(std), _vp(sc)) == OK          # ... and the handle works
    assert np.array_equal(f.X_cols(0, 2 * pb), expand(X, z, z[n - 1], 1))
    assert np.array_equal(std, cd.stdX(f, weighted=True)) and f.w[n - 1] == 0
    sw, sq = C.c_double(), C.c_double()
    assert L.cdh_resid_wmoments(f._h, C.byref(sw), None) == OK and L.cdh_resid_wmoments(f._h, None, C.byref(sq)) == OK
    ls = cd.CDLeastSquaresLoss(y, X)
    assert L.cdh_resid_wmoments(ls._h, C.byref(sw), C.byref(sq)) == BAD                    # not a CDH_WLS handle
    h = C.c_void_p()
    assert L.cdh_create(C.byref(h), cd._lib.CDH_F64, cd._lib.CDH_WLS, n, n, 0, pb, 0) == OK
    assert L.cdh_resid_wmoments(h, C.byref(sw), C.byref(sq)) == BAD                        # no weights set
    assert L.cdh_destroy(h) == OK
    # a row shard: refused, and still a working handle
    assert L.cdh_create(C.byref(h), cd._lib.CDH_F64, cd._lib.CDH_WLS, n, 2 * n, 0, 2 * pb, 0) == OK
    assert L.cdh_set_y(h, _vp(y)) == OK
    assert L.cdh_vc_set_point_loo(h, 0, 0.1, 5, _vp(std), _vp(sc)) == BAD
    assert L.cdh_set_y(h, _vp(y)) == OK
    assert L.cdh_destroy(h) == OK
    f.close(); ls.close()
