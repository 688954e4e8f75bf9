"""cdh_vc_gram (csrc/vc_gram.hpp: k_vc_moments' streamed instantiation on one point, k_vc_moments_reduce) and the locpoly front
ends on the device, against the long-double yardstick of tests/_vc_gram_numpy.py.

Exact sums.  Epanechnikov h = 1 around z0 = 0.5 with z in {0, 0.5, 1}: d in {0, +-0.5}, K in {0.75, 0.5625}.  With |x| <= 3,
|y| <= 4, e in 0 .. 3 every term is a multiple of 2^-14 (K^2: 2^-8, d^6: 2^-6) below 2^5, so every partial sum over fewer
than 2^20 rows is representable in fp64 and the result must EQUAL the true sums whatever the order; the yardstick may then
take its own sums in float64 (asserted: EXACT_ROWS).  Shapes come from the header's own constants (VG.launch) and every case
asserts the branch it is named for.

Rounded data.  Every entry must lie within (L + 2Q + 8) 2^-53 sum_i |term_i| of the yardstick: L additions (the header's
chain length, VG.launch), at most 2Q multiplications for the powers of d, and 8 for K (evaluated by the device's exp: 2),
K^2 (doubles it, plus one), e, the product x x and the fma's own product."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _vc_gram_numpy as VG

pytestmark = pytest.mark.gpu

U64, U32 = 2.0 ** -53, 2.0 ** -24
R, TILE = VG.K["kVgRows"], VG.K["kVgTile"]
EXACT_ROWS = 1 << 20
assert EXACT_ROWS * 2 ** 5 * 2 ** 14 < 2 ** 53
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
KIND = {"gaussian": cd.GaussianKernel, "epanechnikov": cd.EpanechnikovKernel}


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _exact_data(seed, n, p, dtype):
    rng = np.random.default_rng(seed)
    X = rng.integers(1, 4, size=(n, p)) * rng.choice([-1, 1], size=(n, p))
    z = rng.integers(0, 3, size=n) * 0.5
    return (np.asfortranarray(X.astype(dtype)), z.astype(dtype), rng.integers(-4, 5, size=n).astype(dtype),
            rng.integers(0, 4, size=n).astype(dtype))


def _random_data(seed, n, p, dtype):
    rng = np.random.default_rng(seed)
    return (np.asfortranarray(rng.standard_normal((n, p)).astype(dtype)), rng.random(n).astype(dtype),
            rng.standard_normal(n).astype(dtype), (rng.standard_normal(n) ** 2).astype(dtype))


def _eq(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))


def _check_exact(f, X, z, y, e, Q, cols, wpow, use_e, leave_out=None, z0=0.5):
    k = cd.EpanechnikovKernel(1.0)
    G, c, sw = f.expanded_gram(k, z0, leave_out=leave_out, wpow=wpow, e=e if use_e else None, base_cols=cols)
    wG, wc, wsw, _, _ = VG.gram(X, z, y, z0, Q, "epanechnikov", 1.0, wpow, e if use_e else None, leave_out, cols, acc=np.float64)
    tag = (X.shape[0], Q, len(cols), wpow, use_e, leave_out)
    assert _eq(G, wG), ("G", tag, np.argwhere(G != wG)[:5])
    assert _eq(c, wc), ("c", tag)
    assert sw == float(wsw), ("sum w", tag)
    return G, c, sw


# ---- 1. exact sums -----------------------------------------------------------------------------------------------------
ROW_SHAPES = [1, 31, 32, 33, R - 1, R, R + 1, 5 * R + 7]
COL_SHAPES = [1, 2, TILE - 1, TILE, TILE + 1, 63, 64]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q", [0, 1, 2, 3])
def test_exact_sums_at_every_row_and_column_edge(dtype, Q):
    assert R == 64 and TILE == 4 and ROW_SHAPES[-1] < EXACT_ROWS
    seen = set()
    for n in ROW_SHAPES:
        X, z, y, e = _exact_data(1000 * Q + n, n, 64, dtype)
        f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
        for mb in COL_SHAPES:
            la = VG.launch(n, Q, mb)
            seen.add((la["chunks"], la["ragged"]))
            seen.add(("S", la["S"] > 1))
            # the tile edges: mb + 2 columns (y and the ones behind the listed ones) in groups of TILE
            assert la["groups"] == -(-(mb + 2) // TILE) and la["pairs"] * la["S"] <= VG.K["kVgThreads"]
            assert not la["wraps"] and la["G"] == la["chunks"]
            cols = list(range(mb))
            for wpow in (1, 2):
                for use_e in (False, True):
                    _check_exact(f, X, z, y, e, Q, cols, wpow, use_e)
        f.close()
    # one chunk short of a row, exactly one, one and a row; several chunks and a ragged tail; sliced and unsliced pairs
    assert {(1, True), (1, False), (2, True), (6, True), ("S", True), ("S", False)} <= seen


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_sums_when_workgroups_walk_several_chunks(dtype):
    """More chunks than workgroups: capped by kVgMaxBlocks (small records), and by the partial buffer (the largest record)."""
    for Q, mb, p in ((1, 3, 3), (3, 64, 64)):
        G0 = VG.launch(10 ** 7, Q, mb)["G"]
        n = G0 * R + R + 3
        la = VG.launch(n, Q, mb)
        assert la["wraps"] and la["ragged"] and la["chunks"] == G0 + 2 and n < EXACT_ROWS
        assert la["capped_by_blocks"] if mb == 3 else (la["capped_by_buffer"] and la["G"] < VG.K["kVgMaxBlocks"])
        X, z, y, e = _exact_data(77 + Q, n, p, dtype)
        f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
        _check_exact(f, X, z, y, e, Q, list(range(mb)), 2, True)
        f.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q", [0, 2])
def test_exact_sums_of_an_unsorted_subset_with_a_repeat(dtype, Q):
    n, p = 3 * R + 5, 23
    X, z, y, e = _exact_data(5 + Q, n, p, dtype)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    cols = [17, 2, 22, 2, 9, 0]
    G, c, _ = _check_exact(f, X, z, y, e, Q, cols, 1, True)
    Q1 = Q + 1
    assert _eq(G[Q1:2 * Q1], G[3 * Q1:4 * Q1]) and _eq(c[Q1:2 * Q1], c[3 * Q1:4 * Q1])       # the repeated column, twice
    f.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q", [1, 3])
def test_exact_sums_with_a_left_out_row(dtype, Q):
    """First row, last row, the last row of a chunk and the first of the next; and against the full-weight call at the same
    z0 = z[row], which differs by K(0) x_row x_row' at the power-0 entries and nowhere else (d_row = 0)."""
    n, p = 2 * R + 5, 6
    X, z, y, e = _exact_data(31 + Q, n, p, dtype)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    Q1, cols = Q + 1, list(range(p))
    for row in (0, n - 1, R - 1, R):
        G, c, sw = _check_exact(f, X, z, y, e, Q, cols, 1, False, leave_out=row, z0=None)
        Gf, cf, swf = _check_exact(f, X, z, y, e, Q, cols, 1, False, z0=float(z[row]))
        dG, dc = np.zeros_like(G), np.zeros_like(c)
        dG[::Q1, ::Q1] = 0.75 * np.outer(X[row], X[row]).astype(np.float64)
        dc[::Q1] = 0.75 * X[row].astype(np.float64) * float(y[row])
        assert _eq(Gf - G, dG) and _eq(cf - c, dc) and swf - sw == 0.75
        assert np.count_nonzero(Gf - G) == p * p                      # (no x is zero: every power-0 pair moves, nothing else)
    f.close()


# ---- 2. rounded data -----------------------------------------------------------------------------------------------------
def _within(got, want, bound):
    return np.all(np.abs(got.astype(VG.LD) - want) <= bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["gaussian", "epanechnikov"])
@pytest.mark.parametrize("n", [4099, 65537])
def test_rounded_data_within_the_chain_length_bound(dtype, kind, n):
    p, Q, cols, h, z0 = 7, 2, [0, 1, 2, 4, 6], 0.3, 0.45
    X, z, y, e = _random_data(n, n, p, dtype)
    la = VG.launch(n, Q, len(cols))
    assert la["wraps"] == (n == 65537) and la["ragged"]
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    for wpow, ee in ((1, None), (2, e)):
        G, c, sw = f.expanded_gram(KIND[kind](h), z0, wpow=wpow, e=ee, base_cols=cols)
        wG, wc, wsw, aG, ac = VG.gram(X, z, y, z0, Q, kind, h, wpow, ee, None, cols)
        fac = (la["L"] + 2 * Q + 8) * U64
        print(f"vc_gram rounded {np.dtype(dtype).name} {kind} n={n} wpow={wpow}: L={la['L']} max err/bound G "
              f"{float(np.max(np.abs(G - wG) / (fac * aG))):.3f} c {float(np.max(np.abs(c - wc) / (fac * ac))):.3f}")
        assert _within(G, wG, fac * aG) and _within(c, wc, fac * ac) and abs(sw - wsw) <= fac * wsw
    f.close()


def test_the_bound_bites_one_dropped_row_is_a_hundred_bounds_away():
    """At n = 4099 most single rows' terms of an entry exceed 100 x that entry's bound: a dropped or doubled row would be seen."""
    n, p, Q, h, z0 = 4099, 3, 1, 0.3, 0.45
    X, z, y, _ = _random_data(9, n, p, np.float64)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    G, c, _ = f.expanded_gram(cd.GaussianKernel(h), z0)
    f.close()
    wG, wc, _, aG, ac = VG.gram(X, z, y, z0, Q, "gaussian", h)
    fac = (VG.launch(n, Q, p)["L"] + 2 * Q + 8) * U64
    assert _within(G, wG, fac * aG) and _within(c, wc, fac * ac)
    eX, om = VG.expanded(X, z, z0, Q), VG.omega("gaussian", h, z, z0)
    for a, b in ((0, 0), (1, 1), (0, 3), (2, 5), (5, 5)):
        terms = np.abs(om * eX[:, a] * eX[:, b])
        assert int((terms > 100 * fac * aG[a, b]).sum()) > n // 2, (a, b)


# ---- 3. the existing route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q", [1, 2])
def test_agrees_with_set_point_and_gram_weighted(dtype, Q):
    """The bar is the two routes' own bounds added.  cdh_vc_gram: (L + 2Q + 8) u64.  cdh_vc_set_point + cdh_gram_weighted: any order of
    n fp64 additions, n u64; at fp32 storage its columns carry the recurrence v *= d rounded to fp32, at most 2Q roundings per
    product of two of them, its Gram kernel weights an operand in fp32 (1) and keeps fp32 partial sums over chains of 256 rows
    (test_gpu_kernel_sums.GRAMSTEP_F32_CHAIN), and the product itself rounds once: (256 + 2Q + 2) u32.  All times sum |term|."""
    n, p, h, z0 = 5003, 6, 0.35, 0.52
    X, z, y, _ = _random_data(40 + Q, n, p, dtype)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    k = cd.GaussianKernel(h)
    G, c, _ = f.expanded_gram(k, z0)
    f.set_point(k, z0)
    cd._lib.check(f._L.cdh_initialize(f._h, f.p, 0, None, None), f._h)                      # beta = 0: r = y
    ep = f.p
    idx1 = np.arange(1, ep + 1, dtype=np.int64)
    G2, c2 = np.zeros((ep, ep)), np.zeros(ep)
    cd._lib.check(f._L.cdh_gram_weighted(f._h, ep, _vp(idx1), _vp(G2), _vp(c2), None), f._h)
    G3, c3, _ = f.expanded_gram(k, z0)
    assert _eq(G3, G) and _eq(c3, c)                                                   # the expansion in between changed nothing it reads
    f.close()
    _, _, _, aG, ac = VG.gram(X, z, y, z0, Q, "gaussian", h)
    bar = (VG.launch(n, Q, p)["L"] + 2 * Q + 8) * U64 + n * U64
    if dtype == np.float32:
        bar += (256 + 2 * Q + 2) * U32
    bar *= 1 + 1e-6                                                                    # (sum |term| of the rounded columns)
    print(f"vc_gram vs expanded route {np.dtype(dtype).name} Q={Q}: max diff/bar G {float(np.max(np.abs(G - G2) / (bar * aG))):.3f} "
          f"c {float(np.max(np.abs(c - c2) / (bar * ac))):.3f}")
    assert np.all(np.abs(G - G2) <= bar * aG) and np.all(np.abs(c - c2) <= bar * ac)


# ---- 4. read-only --------------------------------------------------------------------------------------------------------
def _state(f):
    beta = np.zeros(f.p)
    cd._lib.check(f._L.cdh_get_beta(f._h, _vp(beta)), f._h)
    return beta.tobytes(), f.w.tobytes(), f.X_cols(0, f.p).tobytes(), np.float64(cd.objective(f)).tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_call_leaves_the_handle_as_it_found_it(dtype):
    n, p, Q = 2003, 5, 2
    X, z, y, e = _random_data(12, n, p, dtype)
    k, opt = cd.EpanechnikovKernel(0.4), cd.CDOptions(maxIter=300, optTol=1e-9, randomize=False, warmStart=True)
    out = []
    for query in (False, True):
        f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
        x = cd.SparseIterate(f.p)
        sx = f.set_point(k, 0.3)
        cd.coordinateDescent_(x, f, cd.ProxL1(0.02, sx), opt)
        before = _state(f)                # (both handles are read the same way: the query is the only difference)
        if query:
            f.expanded_gram(cd.GaussianKernel(0.2), 0.7, wpow=2, e=e, base_cols=[4, 0, 2])
            f.expanded_gram(k, leave_out=n - 1)
        assert _state(f) == before
        cd.coordinateDescent_(x, f, cd.ProxL1(0.01, sx), opt)
        out.append((x.dense().tobytes(), f.last_stats["passes"], f.last_stats["visits"], _state(f)))
        f.close()
    assert out[0] == out[1]


# ---- 5. front ends ---------------------------------------------------------------------------------------------------------
def _scaled_cond(G):
    d = np.sqrt(np.diag(G))
    return np.linalg.cond(G / np.outer(d, d))


def _lstsq_point(X, z, y, z0, Q, kind, h, keep=None):
    from _vc_numpy import expand, weights
    if keep is not None:
        X, z, y = X[keep], z[keep], y[keep]
    sw = np.sqrt(weights(kind, h, z, z0))
    return np.linalg.lstsq(sw[:, None] * expand(X, z, z0, Q), sw * y, rcond=None)[0]


def _solve_bar(X, z, y, z0, Q, kind, h, leave_out=None):
    """4 cond_2(D^-1 G D^-1) times the largest relative entry bound of the rounded-data test, from the yardstick alone."""
    wG, wc, _, aG, ac = VG.gram(X, z, y, z0, Q, kind, h, leave_out=leave_out)
    fac = (VG.launch(X.shape[0], Q, X.shape[1])["L"] + 2 * Q + 8) * U64
    rel = max(float(np.max(fac * aG / np.abs(wG))), float(np.max(fac * ac / np.abs(wc))))
    return 4 * _scaled_cond(wG.astype(np.float64)) * rel


@pytest.mark.parametrize("Q", [0, 1, 2])
def test_locpoly_on_a_grid_against_lstsq(Q):
    from _vc_numpy import gen_data
    X, z, y = gen_data(np.random.default_rng(500), 500, 2, 0)
    zgrid = np.arange(0.01, 0.99, 0.2)
    out = cd.locpoly(X, z, y, zgrid, Q, cd.GaussianKernel(0.4))
    assert out.shape == (2 * (Q + 1), zgrid.shape[0])
    for ind, z0 in enumerate(zgrid):
        bar = _solve_bar(X, z, y, z0, Q, "gaussian", 0.4)
        assert bar <= 1e-9, (Q, z0, bar)                                 # a condition on the inputs, not on the device
        want = _lstsq_point(X, z, y, z0, Q, "gaussian", 0.4)
        assert np.max(np.abs(out[:, ind] - want)) <= bar * np.max(np.abs(want)), (Q, z0)
    one = cd.locpoly(X, z, y, float(zgrid[2]), Q, cd.GaussianKernel(0.4))
    assert _eq(one, out[:, 2])
    if Q == 1:
        f = cd.CDVaryingCoefficientLoss(y, X, z, Q)                      # a resident loss serves as X
        assert _eq(cd.locpoly(f, None, None, zgrid, None, cd.GaussianKernel(0.4)), out)
        f.close()


def test_lvocv_locpoly_against_a_loop_that_deletes_the_row():
    from _vc_numpy import gen_data
    n, Q, hs = 60, 1, [0.3, 0.5]
    X, z, y = gen_data(np.random.default_rng(60), n, 2, 0)
    mse = cd.lvocv_locpoly(X, z, y, Q, hs, cd.GaussianKernel)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    for ih, h in enumerate(hs):
        want, slack = 0.0, 0.0
        for i in range(n):
            keep = np.arange(n) != i
            hb = _lstsq_point(X, z, y, float(z[i]), Q, "gaussian", h, keep)
            bar = _solve_bar(X, z, y, None, Q, "gaussian", h, leave_out=i)
            assert bar <= 1e-9
            G, c, _ = f.expanded_gram(cd.GaussianKernel(h), leave_out=i)
            d = np.sqrt(np.diag(G))
            got = np.linalg.solve(G / np.outer(d, d), c / d) / d
            assert np.max(np.abs(got - hb)) <= bar * np.max(np.abs(hb)), (h, i)
            yh = X[i] @ hb[::Q + 1]
            want += (yh - y[i]) ** 2
            slack += 2 * abs(yh - y[i]) * bar * np.max(np.abs(hb)) * np.abs(X[i]).sum() * 1.01
        assert abs(mse[ih] - want) <= slack + 1e-15 * want, (h, mse[ih], want)
    f.close()


@pytest.mark.parametrize("Q", [0, 1])
def test_standard_errors_against_numpy(Q):
    from _vc_numpy import expand, gen_data, weights
    n, h, z0 = 400, 0.4, 0.55
    X, z, y = gen_data(np.random.default_rng(7), n, 3, 0)
    eps2 = (np.random.default_rng(8).standard_normal(n) ** 2)
    w, eX = weights("gaussian", h, z, z0), expand(X, z, z0, Q)
    A = np.linalg.inv((eX.T * w) @ eX)
    for got, mid in ((cd.getStandardError(X, z, 1.0, z0, Q, cd.GaussianKernel(h)), w * w),
                     (cd.getStandardErrorHEW(X, z, eps2, z0, Q, cd.GaussianKernel(h)), w * w * eps2)):
        want = np.diag(A @ ((eX.T * mid) @ eX) @ A)[::Q + 1]
        assert got.shape == (3,) and np.allclose(got, want, rtol=1e-9, atol=0.0)


def test_refit_locpolyl1_on_a_known_group_support():
    from _vc_numpy import gen_data
    n, Q, h, z0 = 300, 1, 0.4, 0.5
    X, z, y = gen_data(np.random.default_rng(11), n, 2, 4)               # p = 6
    beta = np.zeros(12)
    beta[[3, 8, 9]] = [0.5, -1.0, 2.0]                                   # groups 1 (second coefficient only) and 4
    br, S = cd.refit_locpolyl1(X, z, y, z0, Q, cd.GaussianKernel(h), beta)
    assert S.tolist() == [False, True, False, False, True, False]
    want = _lstsq_point(X[:, S], z, y, z0, Q, "gaussian", h)
    assert br.shape == (4,) and np.allclose(br, want, rtol=1e-9, atol=1e-12)
    x = cd.SparseIterate(12)
    x[4] = 0.5
    br2, S2 = cd.refit_locpolyl1(X, z, y, z0, Q, cd.GaussianKernel(h), x)
    assert S2.tolist() == [False, True, False, False, False, False]
    assert np.allclose(br2, _lstsq_point(X[:, S2], z, y, z0, Q, "gaussian", h), rtol=1e-9, atol=1e-12)
    br0, S0 = cd.refit_locpolyl1(X, z, y, z0, Q, cd.GaussianKernel(h), np.zeros(12))
    assert br0.shape == (0,) and not S0.any()


def test_split_locpoly_against_a_numpy_restatement():
    from _vc_numpy import gen_data
    n, Q, hs = 200, 1, [0.3, 0.6]
    X, z, y = gen_data(np.random.default_rng(21), n, 2, 0)
    Xt, zt, yt = gen_data(np.random.default_rng(22), n, 2, 0)
    zt = 0.05 + 0.9 * zt
    zgrid = np.linspace(0.0, 1.0, 11)
    mse = cd.split_locpoly(X, z, y, Xt, zt, yt, zgrid, Q, hs, cd.GaussianKernel)
    for ih, h in enumerate(hs):
        B = np.stack([_lstsq_point(X, z, y, z0, Q, "gaussian", h) for z0 in zgrid], axis=1)
        want, bi = 0.0, np.zeros(4)
        for i in range(n):
            cd.get_beta_(bi, zgrid, B, zt[i])
            want += (yt[i] - Xt[i] @ bi[::2]) ** 2
        assert abs(mse[ih] - want) <= 1e-8 * want


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_every_documented_refusal_through_the_abi_and_the_api():
    n, p, Q = 50, 3, 1
    X, z, y, e = _random_data(1, n, p, np.float64)
    L, BAD = cd._lib.lib(), cd._lib.CDH_BAD_ARG
    G, c, sw = np.zeros((6, 6)), np.zeros(6), C.c_double()
    idx = np.array([1, 2, 3], dtype=np.int64)

    def call(h, kind=0, bw=0.3, z0=0.5, lo=-1, wpow=1, mb=3, ix=idx, g=G, cc=c):
        return L.cdh_vc_gram(h, kind, bw, z0, lo, wpow, None, mb, _vp(ix), _vp(g), _vp(cc), C.byref(sw))

    plain = cd.CDWeightedLSLoss(y, X, np.ones(n))                        # never given cdh_vc_set_data
    assert call(plain._h) == BAD and b"cdh_vc_set_data" in L.cdh_last_error(plain._h)
    plain.close()
    h = C.c_void_p()
    cd._lib.check(L.cdh_create(C.byref(h), cd._lib.CDH_F64, cd._lib.CDH_WLS, n, n, 0, p * (Q + 1), 0))
    cd._lib.check(L.cdh_vc_set_data(h, p, Q, _vp(X), n, _vp(z)), h)
    assert call(h) == BAD and b"cdh_set_y" in L.cdh_last_error(h)        # out_c before cdh_set_y ...
    assert call(h, cc=None) == cd._lib.CDH_OK                            # ... and without out_c it runs
    cd._lib.check(L.cdh_destroy(h))
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    assert call(f._h) == cd._lib.CDH_OK
    for kw in (dict(mb=0), dict(mb=65, ix=np.ones(65, dtype=np.int64)), dict(ix=np.array([1, 0, 3], dtype=np.int64)),
               dict(ix=np.array([1, 4, 3], dtype=np.int64)), dict(bw=0.0), dict(bw=-0.5), dict(kind=2), dict(wpow=0), dict(wpow=3),
               dict(lo=n), dict(lo=-2), dict(g=None), dict(ix=None)):
        assert call(f._h, **kw) == BAD, kw
    assert L.cdh_vc_gram(None, 0, 0.3, 0.5, -1, 1, None, 3, _vp(idx), _vp(G), _vp(c), None) == BAD
    k = cd.GaussianKernel(0.3)
    for kw in (dict(base_cols=[]), dict(base_cols=[0, 3]), dict(base_cols=[-1]), dict(wpow=3), dict(leave_out=n)):
        with pytest.raises(cd.ArgumentError):
            f.expanded_gram(k, 0.5, **kw)
    with pytest.raises(cd.ArgumentError):
        f.expanded_gram(cd.GaussianKernel(-1.0), 0.5)
    with pytest.raises(TypeError):
        f.expanded_gram("gaussian", 0.5)
    with pytest.raises(cd.DimensionMismatch):
        f.expanded_gram(k, 0.5, e=e[:-1])
    G1, c1, s1 = f.expanded_gram(k, 0.5)                                 # the handle stays usable after every refusal
    assert np.all(np.isfinite(G1)) and s1 > 0
    f.close()


def test_row_sharded_handles_are_refused():
    n, p, Q = 40, 2, 0
    X, z, _, _ = _random_data(2, n, p, np.float64)
    L = cd._lib.lib()
    h = C.c_void_p()
    cd._lib.check(L.cdh_create(C.byref(h), cd._lib.CDH_F64, cd._lib.CDH_WLS, n, 2 * n, 0, p, 0))     # half of the rows of a sharded problem
    G, idx = np.zeros((2, 2)), np.array([1, 2], dtype=np.int64)
    assert L.cdh_vc_gram(h, 0, 0.3, 0.5, -1, 1, None, 2, _vp(idx), _vp(G), None, None) == cd._lib.CDH_BAD_ARG
    assert b"row-sharded" in L.cdh_last_error(h)
    cd._lib.check(L.cdh_destroy(h))


# ---- 7. bit-identical ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_calls_agree_bit_for_bit(dtype):
    n, p, Q = 70001, 10, 2
    X, z, y, e = _random_data(3, n, p, dtype)
    outs = []
    for _ in range(2):
        f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
        a = f.expanded_gram(cd.GaussianKernel(0.25), 0.4, wpow=2, e=e)
        b = f.expanded_gram(cd.GaussianKernel(0.25), 0.4, wpow=2, e=e)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
        outs.append(a)
        f.close()
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
