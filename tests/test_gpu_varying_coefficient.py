"""The varying-coefficient lasso on the device: cdh_vc_set_data / cdh_vc_set_point (k_vc_weights, k_vc_expand, k_vc_reduce),
cdh_col_wrms, cdh_gram_weighted and locpolyl1 on top of them, held to the numpy restatement in tests/_vc_numpy.py (pinned
against the reference's own checks in tests/test_vc_host.py) and to `oracle`'s CDWeightedLSLoss and driver."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
from _vc_numpy import expand, gen_data, oracle_locpolyl1, peak, weights, wstd

pytestmark = pytest.mark.gpu

U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
KERNELS = {"gaussian": cd.GaussianKernel, "epanechnikov": cd.EpanechnikovKernel}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _problem(seed, n, pb, dtype):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, pb)).astype(dtype))
    z = rng.random(n).astype(dtype)
    y = rng.standard_normal(n).astype(dtype)
    return X, z, y


# ---- 1. the expansion, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", [1, 37, 64])
@pytest.mark.parametrize("n", [33, 500, 1237, 300_000])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_expansion_is_bit_identical_to_the_recurrence(dtype, n, pb):
    """v = x; v *= (z - z0) is a plain multiply stored to memory: no room for contraction, so equality is the test.
    n = 33: pad rows; 500 / 1237: tail vectors; 300 000: several grid-stride iterations per thread."""
    X, z, y = _problem(n + pb, n, pb, dtype)
    for degree in range(4):
        f = cd.CDVaryingCoefficientLoss(y, X, z, degree)
        ep = pb * (degree + 1)
        assert f.p == ep
        for kern, z0 in ((cd.GaussianKernel(0.1), 0.3), (cd.EpanechnikovKernel(0.25), 0.7)):
            f.set_point(kern, z0)
            got = f.X_cols(0, ep)
            assert got.dtype == X.dtype
            assert np.array_equal(got, expand(X, z, z0, degree)), (degree, z0)
        assert np.array_equal(got[:, ::degree + 1], X)      # the base columns survive two points with different z0
        f.close()


# ---- 2. the weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h", [("gaussian", 0.1), ("gaussian", 1.0), ("epanechnikov", 0.25)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_weights_against_numpy(dtype, kind, h):
    """Both sides evaluate K in double on the same stored z and the same z0 and round once to T.  Gaussian: the arguments
    -(d d) / h are identical (one multiply, one division, both correctly rounded), the two exp implementations are each
    within 1 ulp of the truth, the division by h is correctly rounded on both sides: the results differ by at most
    ~2.5 u_64 K, and after the rounding to T by at most 1 ulp_T of a value <= K(0) -- inside 4 u_T K(0).  Epanechnikov: u is
    the same correctly rounded quotient on both sides, so the zeros (|u| >= 1) agree exactly; 1 - u u may be contracted to
    an fma on the device, an absolute difference of at most u_64 before the scaling by 0.75 / h = K(0): again inside
    4 u_T K(0) after rounding to T."""
    n = 1237
    X, z, y = _problem(7, n, 3, dtype)
    f = cd.CDVaryingCoefficientLoss(y, X, z, 1)
    bound = 4 * U[np.dtype(dtype)] * peak(kind, h)
    for z0 in (0.1, 0.5, 0.9):
        f.set_point(KERNELS[kind](h), z0)
        got, want = f.w, weights(kind, h, z, z0)
        err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
        print(f"weights {kind} h={h} {np.dtype(dtype).name} z0={z0}: max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        if kind == "epanechnikov":
            nz = int((want == 0).sum())
            print(f"  exact zeros: {nz} of {n}")
            assert 200 <= nz <= n - 200 and np.array_equal(got == 0, want == 0)    # both branches well populated
    f.close()


# ---- 3. the weighted column scales ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pb,degree", [(33, 1, 3), (1237, 37, 2), (500, 64, 1), (300_000, 64, 2), (1237, 5, 0)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_weighted_column_scales(dtype, n, pb, degree):
    """set_point's stdX and cdh_col_wrms take the same sums in the same order: equal to the bit, and run to run.  Against
    a long-double sum of the same stored values: every term w x^2 is non-negative, so n 2^-53 relative bounds what any
    order of summation in double can lose (the argument of tests/test_gpu_kernel_sums.py); the square root halves it."""
    X, z, y = _problem(11 * n + degree, n, pb, dtype)
    f = cd.CDVaryingCoefficientLoss(y, X, z, degree)
    kern, z0 = cd.GaussianKernel(0.1), 0.4
    s1 = f.set_point(kern, z0)
    s2 = cd.stdX(f, weighted=True)
    assert np.array_equal(s1, s2)
    f.set_point(cd.EpanechnikovKernel(0.3), 0.8)
    assert np.array_equal(f.set_point(kern, z0), s1)                      # run to run, after another point in between
    g = cd.CDVaryingCoefficientLoss(y, X, z, degree)
    assert np.array_equal(g.set_point(kern, z0), s1)                      # ... and on a fresh handle
    want = wstd(weights("gaussian", 0.1, z, z0), expand(X, z, z0, degree))
    rel = float(np.max(np.abs(s1 - want) / want))
    print(f"wstd n={n} p={pb}x{degree + 1} {np.dtype(dtype).name}: max rel err {rel:.3e} (bound {n * 2.0 ** -53:.3e})")
    assert rel <= n * 2.0 ** -53
    f.close(); g.close()


# ---- 4. locpolyl1 against the oracle ----------------------------------------------------------------------------------
OPTS = dict(maxIter=2000, optTol=1e-12, randomize=False)
_REF = gen_data(np.random.default_rng(1), 500, 10, 40)     # test/varying_coefficient_lasso.jl:121-142, benchmark/locpoly_bench.jl:156-169
CASES = {
    "ref-d0": (_REF, 0, "gaussian", 0.1, 0.05, np.arange(0.01, 0.99, 0.1)),
    "ref-d1": (_REF, 1, "gaussian", 0.1, 0.05, np.arange(0.01, 0.99, 0.1)),
    "ref-d2": (_REF, 2, "gaussian", 0.1, 0.05, np.arange(0.21, 0.815, 0.1)),
    "epan-37": (gen_data(np.random.default_rng(2), 1237, 10, 27), 2, "epanechnikov", 0.25, 0.05, np.array([0.1, 0.5, 0.9])),
    "one-d3": (gen_data(np.random.default_rng(3), 500, 1, 0), 3, "gaussian", 0.1, 0.05, np.array([0.3, 0.5, 0.7])),
}
_oracle_cache = {}


def _large_case():
    return gen_data(np.random.default_rng(4), 300_000, 10, 54), 2, "gaussian", 0.05, 0.02, np.array([0.2, 0.4, 0.6, 0.8])


def _oracle(name, case, dtype=np.float64):
    key = (name, np.dtype(dtype).name)
    if key not in _oracle_cache:
        (X, z, y), degree, kind, h, lam0, zgrid = case
        _oracle_cache[key] = oracle_locpolyl1(O, X.astype(dtype), z.astype(dtype), y.astype(dtype), zgrid, degree, kind, h,
                                              lam0, **OPTS)
    return _oracle_cache[key]


def _gpu(case, dtype=np.float64, setup=None, refit=False, opts=OPTS):
    (X, z, y), degree, kind, h, lam0, zgrid = case
    f = cd.CDVaryingCoefficientLoss(y.astype(dtype), X.astype(dtype), z.astype(dtype), degree)
    if setup:
        setup(f)
    out, outR = cd.locpolyl1(f, None, None, zgrid, degree, KERNELS[kind](h), lam0, refit, cd.CDOptions(**opts))
    return f, out, outR


def _check_parity(name, case, f, out, tol, dtype=np.float64, coord=False):
    want, stats, orders = _oracle(name, case, dtype)
    zgrid = case[-1]
    assert len(f.point_stats) == len(zgrid)
    for i, z0 in enumerate(zgrid):
        err = float(np.max(np.abs(out[:, i] - want[:, i])))
        print(f"{name} z0={z0:.2f}: oracle passes {stats[i]['passes']} nnz {len(orders[i])}; gpu passes "
              f"{f.point_stats[i]['passes']}; max|dbeta| {err:.3e} (tol {tol:g})")
        assert stats[i]["converged"] and f.point_stats[i]["converged"], (name, z0)
        assert err <= tol, (name, z0, err)
        if coord:
            assert f.point_stats[i]["passes"] == stats[i]["passes"], (name, z0)
            assert np.array_equal(f.point_stats[i]["support"], orders[i]), (name, z0)


@pytest.mark.parametrize("name", list(CASES))
def test_locpolyl1_parity_default_sweep(name):
    f, out, _ = _gpu(CASES[name], setup=lambda f: f.set_onchip_solve(False))     # (the suite's CDH_SMALL_PATH=0, spelled out)
    assert f.onchip_stats()["solves"] == 0
    _check_parity(name, CASES[name], f, out, 1e-10)


@pytest.mark.parametrize("name", list(CASES))
def test_locpolyl1_parity_coord_sweep_same_passes_and_support_order(name):
    f, out, _ = _gpu(CASES[name], setup=lambda f: f.set_sweep_mode("coord"))
    _check_parity(name, CASES[name], f, out, 1e-10, coord=True)


@pytest.mark.parametrize("name", ["ref-d0", "ref-d1", "ref-d2", "one-d3"])
def test_locpolyl1_parity_one_launch_solve(name):
    """Every grid point must see a fresh Gram matrix: a missed invalidation would solve the previous point's problem."""
    f, out, _ = _gpu(CASES[name], setup=lambda f: f.set_onchip_solve(True))
    st = f.onchip_stats()
    n_points = len(CASES[name][-1])
    assert st["solves"] >= n_points and st["gram_matrices"] == n_points, st
    _check_parity(name, CASES[name], f, out, 1e-10)


@pytest.mark.parametrize("name", list(CASES))
def test_locpolyl1_parity_gradient_cache_from_the_first_pass(name):
    """... and a fresh gradient cache: its Gram columns belong to one point's design and weights."""
    f, out, _ = _gpu(CASES[name], setup=lambda f: f.set_gradient_cache(3))
    cs = f.cache_stats()
    print(f"{name}: cache {cs}")
    if name == "epan-37":              # a sparse support (20 of 111): the cache does serve passes here
        assert cs["passes"] > 0 and cs["gram_columns"] > 0
    _check_parity(name, CASES[name], f, out, 1e-10)


@pytest.mark.parametrize("name", ["ref-d1", "epan-37"])
def test_locpolyl1_parity_fp32_storage(name):
    """fp32 storage against the fp64 oracle on the fp32-rounded inputs (weights and expansion as the device forms them,
    in fp32): DESIGN section 2's 3e-4.  The oracle keeps optTol = 1e-12; the device stops at 1e-6, the setting of every fp32
    solve in tests/test_gpu_parity.py: a residual stored in fp32 is rounded at 2^-24 ~ 6e-8 relative at every visit, so
    steps never fall below that scale and a 1e-12 stopping rule cannot be met by the number format."""
    f, out, _ = _gpu(CASES[name], dtype=np.float32, opts=dict(OPTS, optTol=1e-6))
    _check_parity(name, CASES[name], f, out, 3e-4, dtype=np.float32)


def test_locpolyl1_parity_large():
    case = _large_case()
    f, out, _ = _gpu(case)
    _check_parity("large", case, f, out, 1e-10)


def test_changing_only_z0_back_and_forth_returns_the_first_solution():
    (X, z, y), degree, kind, h, lam0, _ = CASES["ref-d1"]
    for setup in (None, lambda f: f.set_onchip_solve(True), lambda f: f.set_gradient_cache(3)):
        f = cd.CDVaryingCoefficientLoss(y, X, z, degree)
        if setup:
            setup(f)
        out, _ = cd.locpolyl1(f, None, None, [0.31, 0.61, 0.31, 0.61], degree, KERNELS[kind](h), lam0, False, cd.CDOptions(**OPTS))
        assert all(s["converged"] for s in f.point_stats)
        assert np.max(np.abs(out[:, 0] - out[:, 1])) > 1e-3               # the two points do differ
        assert np.max(np.abs(out[:, 2] - out[:, 0])) <= 1e-10
        assert np.max(np.abs(out[:, 3] - out[:, 1])) <= 1e-10
        f.close()


# ---- 5. the refit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_refit_solves_the_weighted_normal_equations_on_the_support(name):
    """outR against numpy's solution of (Xs'W Xs) b = Xs'W y on the device's own support.  The device forms
    b = beta_S + G^-1 c from a Gram block whose entries carry the rounding of sums over n rows (~log2 n levels of pairwise
    partials) and solves an |S| x |S| system scaled to unit diagonal: allowed 4 kappa (|S| + log2 n) 2^-53 |b|_inf with
    kappa the 2-norm condition number of that scaled block."""
    case = CASES[name]
    (X, z, y), degree, kind, h, lam0, zgrid = case
    f, out, outR = _gpu(case, refit=True)
    n = X.shape[0]
    for i, z0 in enumerate(zgrid):
        S = cd.get_nonzero_coordinates(out[:, i], X.shape[1], degree, True)
        assert S.any() and not outR[~S, i].any()
        w = weights(kind, h, z, z0).astype(np.longdouble)
        Xs = expand(X, z, z0, degree)[:, S].astype(np.longdouble)
        G = (Xs.T * w) @ Xs
        c = (Xs.T * w) @ y.astype(np.longdouble)
        d = np.sqrt(np.diag(G))
        Gs = (G / np.outer(d, d)).astype(np.float64)
        kappa = float(np.linalg.cond(Gs))
        assert kappa <= 1e5, kappa
        b = np.linalg.solve(Gs, (c / d).astype(np.float64)) / d.astype(np.float64)
        allowed = 4 * kappa * (S.sum() + np.log2(n)) * 2.0 ** -53 * float(np.max(np.abs(b)))
        err = float(np.max(np.abs(outR[S, i] - b)))
        print(f"refit {name} z0={z0:.2f}: |S|={S.sum()} kappa={kappa:.3g} err {err:.3e} allowed {allowed:.3e}")
        assert allowed < 1e-8 and err <= allowed


@pytest.mark.parametrize("m", [5, 64, 100])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gram_weighted_is_exact_on_summable_integers_and_cdh_gram_is_unchanged(dtype, m):
    """Small integers: every product and partial sum is representable (fp32 storage: |x| <= 127, w <= 3, |y| <= 511 keep the
    matrix pipe's 256-row fp32 partials below 2^24, as tests/test_gpu_kernel_sums.py derives), so X_S'W X_S, X_S'W r and r'W r
    must equal numpy's to the bit whatever the order."""
    rng = np.random.default_rng(m)
    n, p = 5003, 120
    xmax, ymax = (2047, 2047) if dtype == np.float64 else (127, 511)
    X = np.asfortranarray(rng.integers(-xmax, xmax + 1, size=(n, p)).astype(dtype))
    y = rng.integers(-ymax, ymax + 1, size=n).astype(dtype)
    w = rng.integers(0, 4, size=n).astype(dtype)
    f = cd.CDWeightedLSLoss(y, X, w)
    idx1 = np.ascontiguousarray(rng.permutation(p)[:m] + 1, dtype=np.int64)
    G, c, q = np.zeros((m, m)), np.zeros(m), C.c_double()
    cd.check(f._L.cdh_gram_weighted(f._h, m, _vp(idx1), _vp(G), _vp(c), C.byref(q)), f._h)
    Xs, wl, yl = X[:, idx1 - 1].astype(np.float64), w.astype(np.float64), y.astype(np.float64)
    assert np.array_equal(G, (Xs.T * wl) @ Xs)
    assert np.array_equal(c, (Xs.T * wl) @ yl) and q.value == float((wl * yl) @ yl)
    G0, c0, q0 = np.zeros((m, m)), np.zeros(m), C.c_double()
    cd.check(f._L.cdh_gram(f._h, m, _vp(idx1), _vp(G0), _vp(c0), C.byref(q0)), f._h)
    assert np.array_equal(G0, Xs.T @ Xs) and np.array_equal(c0, Xs.T @ yl) and q0.value == float(yl @ yl)
    f.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------
def test_documented_statuses_and_the_handle_stays_usable():
    L = cd._lib.lib()
    BAD, DIM, OK = cd._lib.CDH_BAD_ARG, cd._lib.CDH_DIM_MISMATCH, cd._lib.CDH_OK
    n, pb = 200, 3
    X, z, y = _problem(5, n, pb, np.float64)
    std = np.zeros(2 * pb)
    f = cd.CDWeightedLSLoss(y, np.asfortranarray(np.zeros((n, 2 * pb))), np.ones(n))
    assert L.cdh_vc_set_point(f._h, 0, 0.1, 0.5, _vp(std)) == BAD                     # before cdh_vc_set_data
    assert L.cdh_vc_set_data(f._h, pb, 2, _vp(X), n, _vp(z)) == DIM                   # p != p_base (degree + 1)
    assert L.cdh_vc_set_data(f._h, pb, 4, _vp(X), n, _vp(z)) == BAD                   # degree 4
    assert L.cdh_vc_set_data(f._h, pb, -1, _vp(X), n, _vp(z)) == BAD
    assert L.cdh_vc_set_data(f._h, pb, 1, _vp(X), n, _vp(z)) == OK
    assert L.cdh_vc_set_point(f._h, 0, 0.0, 0.5, _vp(std)) == BAD                     # bandwidth 0
    assert L.cdh_vc_set_point(f._h, 0, -1.0, 0.5, _vp(std)) == BAD
    assert L.cdh_vc_set_point(f._h, 7, 0.1, 0.5, _vp(std)) == BAD                     # unknown kernel
    assert b"kernel" in L.cdh_last_error(f._h)
    assert L.cdh_vc_set_point(f._h, 0, 0.1, 0.5, None) == OK                          # out_std may be NULL
    assert L.cdh_vc_set_point(f._h, 1, 0.25, 0.5, _vp(std)) == OK                     # ... and the handle works
    assert np.array_equal(f.X_cols(0, 2 * pb), expand(X, z, 0.5, 1))
    assert np.array_equal(std, cd.stdX(f, weighted=True))
    ls = cd.CDLeastSquaresLoss(y, X)
    assert L.cdh_vc_set_data(ls._h, pb, 0, _vp(X), n, _vp(z)) == DIM                  # not a CDH_WLS handle
    assert L.cdh_col_wrms(ls._h, _vp(std)) == BAD and L.cdh_get_obs_weights(ls._h, _vp(np.zeros(n))) == BAD
    assert np.all(cd.stdX(ls) > 0)
    # a row shard: refused by both calls, and still a working handle
    h = C.c_void_p()
    assert L.cdh_create(C.byref(h), cd._lib.CDH_F64, cd._lib.CDH_WLS, n, 2 * n, 0, 2 * pb, 0) == OK
    assert L.cdh_vc_set_data(h, pb, 1, _vp(X), n, _vp(z)) == BAD
    assert b"shard" in L.cdh_last_error(h)
    assert L.cdh_vc_set_point(h, 0, 0.1, 0.5, _vp(std)) == BAD
    assert L.cdh_set_y(h, _vp(y)) == OK
    assert L.cdh_destroy(h) == OK
    f.close(); ls.close()
