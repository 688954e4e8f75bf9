"""cdh_vc_gram_batch (csrc/vc_gram.hpp: k_vc_moments) on the device.  The export promises that point t of a batch IS
cdh_vc_gram at that point, addition for addition, so the yardstick of most tests here is the single-point export itself,
compared with tobytes() and no tolerance; tests/test_gpu_vc_gram.py pins that export to the long-double yardstick.  The two
exports run one body, and cdh_vc_gram always launches k_vc_moments' streamed instantiation on one point: in the streamed cases
batch and single are the same code, in the resident cases (and wherever the shared scratch could carry state from one call to
the next: section 2b) they are two code paths compared byte for byte.  The exact sums of section 3 go straight to the
yardstick (tests/_vc_gram_numpy.py) with the exactness argument of that file: every term a multiple of 2^-14 below 2^5,
fewer than 2^20 rows.  Shapes come from the plan restated in tests/_vc_gram_batch_plan.py and every case asserts the regime it
is named for."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _vc_gram_batch_plan as BP
import _vc_gram_numpy as VG
from test_gpu_vc_gram import _exact_data, _random_data, _state, _vp

pytestmark = pytest.mark.gpu

R = VG.K["kVgRows"]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
KIND = {"gaussian": cd.GaussianKernel, "epanechnikov": cd.EpanechnikovKernel}
FAR = 5.0            # z lies in [0, 1): no row is within a bandwidth below 4 of this point


def _same(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _points(n, z, hs=(0.3, 0.45)):
    """A mixed batch: plain points (the first two at a stored z, so that their support holds a row whatever n is), a point
    whose Epanechnikov support is empty between them, the left-out rows 0, n - 1 and, where they exist, 63 and 64; two
    bandwidths, alternating.  -> (h, z0, leave_out) as vectors."""
    z0 = [float(z[0]), FAR, float(z[n - 1])]
    lo = [-1, -1, -1]
    for row in sorted({0, n - 1} | {r for r in (R - 1, R) if r < n}):
        z0.append(0.0)
        lo.append(row)
    z0.append(0.55)
    lo.append(-1)
    h = [hs[t % 2] for t in range(len(z0))]
    return np.array(h), np.array(z0), np.array(lo, dtype=np.int64)


def _check_against_single(f, kind, h, z0, lo, **kw):
    """Every point of the batch against cdh_vc_gram at that point, byte for byte.  -> the batch's outputs."""
    G, c, sw = f.expanded_gram_batch(KIND[kind], h, z0, leave_out=lo, **kw)
    assert G.shape[0] == h.shape[0] == c.shape[0] == sw.shape[0]
    for t in range(h.shape[0]):
        G1, c1, s1 = f.expanded_gram(KIND[kind](float(h[t])), float(z0[t]), leave_out=None if lo[t] < 0 else int(lo[t]), **kw)
        tag = (f.n, f.degree, kind, t, float(h[t]), float(z0[t]), int(lo[t]), sorted(kw))
        assert _same(G[t], G1), ("G", tag, np.argwhere(G[t] != G1)[:5])
        assert _same(c[t], c1), ("c", tag)
        assert _same(sw[t], s1), ("sum w", tag)
    return G, c, sw


# ---- 1. bit for bit against cdh_vc_gram ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["gaussian", "epanechnikov"])
def test_resident_regime_is_the_single_point_export_bit_for_bit(dtype, Q, kind):
    for n in (1, R - 1, R, R + 1, 5 * R + 7):
        X, z, y, e = _random_data(100 * Q + n, n, 64, dtype)
        f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
        h, z0, lo = _points(n, z)
        for mb in (1, 3, 4, 5, 63, 64):
            pl, la = BP.plan(n, Q, mb, h.shape[0]), VG.launch(n, Q, mb)
            assert pl["resident"] and len(pl["groups"]) == 1 and pl["G"] == la["chunks"]
            assert (la["S"] > 1) == (mb <= 5)                        # sliced pairs, unsliced pairs, and the tile edge 3 | 4 | 5
            kw = dict(wpow=2, e=e) if mb == 5 else {}
            G, c, sw = _check_against_single(f, kind, h, z0, lo, base_cols=list(range(mb)), **kw)
            if kind == "epanechnikov":                               # the point without support, between two ordinary ones
                assert not G[1].any() and not c[1].any() and sw[1] == 0.0 and sw[0] > 0.0 and sw[2] > 0.0
        f.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["gaussian", "epanechnikov"])
@pytest.mark.parametrize("Q,mb", [(1, 3), (3, 64)])
def test_streamed_regime_is_the_single_point_export_bit_for_bit(dtype, kind, Q, mb):
    """The two wrap shapes of test_exact_sums_when_workgroups_walk_several_chunks: capped by kVgMaxBlocks, and by the partial buffer."""
    G0 = VG.launch(10 ** 7, Q, mb)["G"]
    n = G0 * R + R + 3
    la = VG.launch(n, Q, mb)
    assert la["wraps"] and la["ragged"] and (la["capped_by_blocks"] if mb == 3 else la["capped_by_buffer"])
    X, z, y, e = _random_data(7 + Q, n, mb, dtype)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    h, z0, lo = _points(n, z)
    h, z0, lo = np.append(h, 0.3), np.append(z0, 0.2), np.append(lo, -1)     # a ninth point
    pl = BP.plan(n, Q, mb, h.shape[0])
    assert h.shape[0] == 9 and not pl["resident"] and pl["groups"][0]["grid_y"] == pl["groups"][0]["pts"]
    # the largest records: eight points fill the partial buffer and the ninth is a launch group of its own
    assert [g["pts"] for g in pl["groups"]] == ([8, 1] if mb == 64 else [9])
    G, c, sw = _check_against_single(f, kind, h, z0, lo, wpow=2, e=e)
    if kind == "epanechnikov":
        assert not G[1].any() and not c[1].any() and sw[1] == 0.0 and sw[0] > 0.0 and sw[2] > 0.0
    f.close()


# ---- 2. a point does not depend on its batch -------------------------------------------------------------------------------
def test_a_points_bytes_do_not_depend_on_where_it_stands():
    """Q = 3, mb = 64: a record is 14 817 doubles, so a launch group holds few points and points-per-group + 1 is small."""
    n, Q, mb = 2 * R + 2, 3, 64
    X, z, y, _ = _random_data(21, n, mb, np.float64)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    k, probe = cd.GaussianKernel, (0.37, 0.41)                       # (h, z0) of the point that is followed around
    want = f.expanded_gram(k(probe[0]), probe[1])
    pg = BP.plan(n, Q, mb, 1)["group_points"]
    assert VG.nrec(Q, mb) == 14817 and pg < 300
    rng = np.random.default_rng(5)

    def batch(m, at):
        h, z0 = 0.2 + 0.5 * rng.random(m), rng.random(m)
        lo = np.where(rng.random(m) < 0.3, rng.integers(0, n, size=m), -1)
        for t in at:
            h[t], z0[t], lo[t] = probe[0], probe[1], -1
        G, c, sw = f.expanded_gram_batch(k, h, z0, leave_out=lo)
        for t in at:
            assert _same(G[t], want[0]) and _same(c[t], want[1]) and _same(sw[t], want[2]), (m, t)

    batch(1, [0])                                                    # alone
    m = pg + 1                                                       # two launch groups: pg points and one
    pl = BP.plan(n, Q, mb, m)
    assert pl["resident"] and [g["pts"] for g in pl["groups"]] == [pg, 1]
    per = pl["groups"][0]["per"]
    assert pl["groups"][0]["grid_y"] > 2 and per >= 2
    # first; both sides of the first share edge (the last point of share 0, the first of share 1) and of the second; the
    # last point of the first launch group; the second group's only point, which is the batch's last
    batch(m, [0, per - 1, per, 2 * per - 1, 2 * per, pg - 1, pg])
    m2 = 3 * BP.K["kVgbMinSharePoints"] + 1                          # a short batch: other shares, other edges
    pl2 = BP.plan(n, Q, mb, m2)["groups"]
    assert len(pl2) == 1 and pl2[0]["grid_y"] == 3 and pl2[0]["edges"][-2] < m2 - 1
    e1 = pl2[0]["edges"][1]
    batch(m2, [0, e1 - 1, e1, e1 + 1, m2 - 1])
    f.close()


# ---- 2b. the two exports share a scratch and leave nothing in it for each other ------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q,mb,wpow,kind", [(1, 5, 2, "gaussian"), (3, 64, 1, "epanechnikov")])
def test_single_and_batch_calls_on_one_handle_leave_each_other_nothing(dtype, Q, mb, wpow, kind):
    """n = 65: two chunks, the second of one row.  The single-point call keeps its point behind the columns in one block, the
    batch has a point list of its own, and both read the columns and e from the same buffers: a single call after a batch must
    not see the batch's e or a stale point, and a batch after a single call must not depend on it."""
    n = R + 1
    X, z, y, e = _random_data(40 + Q, n, mb, dtype)
    h, z0, lo = _points(n, z)
    h, z0, lo = np.append(h, [0.45, 0.3]), np.append(z0, [0.2, 0.8]), np.append(lo, [-1, -1])
    assert h.shape[0] == 9 and {0, R - 1, R} <= set(lo.tolist()) and lo[0] == -1
    pl = BP.plan(n, Q, mb, 9)
    assert pl["resident"] and pl["G"] == 2 and len(pl["groups"]) == 1 and (VG.launch(n, Q, mb)["S"] > 1) == (mb == 5)
    k0 = KIND[kind](float(h[0]))

    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    first = f.expanded_gram(k0, float(z0[0]), wpow=wpow)
    batch = f.expanded_gram_batch(KIND[kind], h, z0, leave_out=lo, wpow=wpow, e=e)
    again = f.expanded_gram(k0, float(z0[0]), wpow=wpow)
    with_e = f.expanded_gram(k0, float(z0[0]), wpow=wpow, e=e)
    f.close()
    assert all(_same(u, v) for u, v in zip(again, first))            # neither the batch's e nor a stale point is picked up
    assert not _same(with_e[0], first[0])                            # (e does change the result)
    assert all(_same(u[0], v) for u, v in zip(batch, with_e))        # the resident batch's entry is the streamed single point

    g = cd.CDVaryingCoefficientLoss(y, X, z, Q)                      # a fresh handle: the batch first, then the single point
    batch2 = g.expanded_gram_batch(KIND[kind], h, z0, leave_out=lo, wpow=wpow, e=e)
    first2 = g.expanded_gram(k0, float(z0[0]), wpow=wpow)
    with_e2 = g.expanded_gram(k0, float(z0[0]), wpow=wpow, e=e)
    g.close()
    assert all(_same(u, v) for u, v in zip(batch2, batch))
    assert all(_same(u, v) for u, v in zip(first2, first)) and all(_same(u, v) for u, v in zip(with_e2, with_e))


# ---- 3. exact sums against the yardstick -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", ["resident", "streamed"])
def test_exact_sums_of_a_batch_against_the_yardstick(dtype, regime):
    Q, mb = (2, 6) if regime == "resident" else (1, 3)
    n = 5 * R + 7 if regime == "resident" else VG.K["kVgMaxBlocks"] * R + R + 3
    assert n < 1 << 20
    X, z, y, e = _exact_data(3 + Q, n, mb, dtype)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    z0 = np.array([0.0, 0.5, 1.0, 0.0, 0.0])
    lo = np.array([-1, -1, -1, R, n - 1], dtype=np.int64)
    assert BP.plan(n, Q, mb, 5)["resident"] == (regime == "resident")
    G, c, sw = f.expanded_gram_batch(cd.EpanechnikovKernel, 1.0, z0, leave_out=lo, wpow=2, e=e)
    f.close()
    for t in range(5):
        wG, wc, wsw, _, _ = VG.gram(X, z, y, z0[t], Q, "epanechnikov", 1.0, 2, e, None if lo[t] < 0 else int(lo[t]), None, acc=np.float64)
        assert np.array_equal(G[t], wG) and np.array_equal(c[t], wc) and sw[t] == float(wsw), (regime, t)


# ---- 4. read-only --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_batch_call_leaves_the_handle_as_it_found_it(dtype):
    n, p, Q = 2003, 5, 2
    X, z, y, e = _random_data(12, n, p, dtype)
    k, opt = cd.EpanechnikovKernel(0.4), cd.CDOptions(maxIter=300, optTol=1e-9, randomize=False, warmStart=True)
    out = []
    for query in (False, True):
        f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
        x = cd.SparseIterate(f.p)
        sx = f.set_point(k, 0.3)
        cd.coordinateDescent_(x, f, cd.ProxL1(0.02, sx), opt)
        before = _state(f)
        if query:
            f.expanded_gram_batch(cd.GaussianKernel, [0.2, 0.3, 0.25], [0.7, 0.1, 0.5], wpow=2, e=e, base_cols=[4, 0, 2])
            f.expanded_gram_batch(cd.EpanechnikovKernel, 0.4, leave_out=np.arange(n - 40, n))
        assert _state(f) == before
        cd.coordinateDescent_(x, f, cd.ProxL1(0.01, sx), opt)
        out.append((x.dense().tobytes(), f.last_stats["passes"], f.last_stats["visits"], _state(f)))
        f.close()
    assert out[0] == out[1]


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_every_documented_refusal_through_the_abi_and_the_api():
    n, p, Q, m = 50, 3, 1, 4
    X, z, y, e = _random_data(1, n, p, np.float64)
    L, BAD = cd._lib.lib(), cd._lib.CDH_BAD_ARG
    G, c, sw = np.zeros((m, 6, 6)), np.zeros((m, 6)), np.zeros(m)
    idx = np.array([1, 2, 3], dtype=np.int64)
    H, Z0, LO = np.full(m, 0.3), np.linspace(0.2, 0.8, m), np.array([-1, 7, -1, n - 1], dtype=np.int64)

    def call(h, kind=0, m=m, bw=H, z0=Z0, lo=LO, wpow=1, mb=3, ix=idx, g=G, cc=c):
        return L.cdh_vc_gram_batch(h, kind, m, _vp(bw), _vp(z0), _vp(lo), wpow, None, mb, _vp(ix), _vp(g), _vp(cc), _vp(sw))

    plain = cd.CDWeightedLSLoss(y, X, np.ones(n))                        # never given cdh_vc_set_data
    assert call(plain._h) == BAD and b"cdh_vc_set_data" in L.cdh_last_error(plain._h)
    plain.close()
    h = C.c_void_p()
    cd._lib.check(L.cdh_create(C.byref(h), cd._lib.CDH_F64, cd._lib.CDH_WLS, n, n, 0, p * (Q + 1), 0))
    cd._lib.check(L.cdh_vc_set_data(h, p, Q, _vp(X), n, _vp(z)), h)
    assert call(h) == BAD and b"cdh_set_y" in L.cdh_last_error(h)        # out_c before cdh_set_y ...
    assert call(h, cc=None) == cd._lib.CDH_OK                            # ... and without out_c it runs
    cd._lib.check(L.cdh_destroy(h))
    h = C.c_void_p()
    cd._lib.check(L.cdh_create(C.byref(h), cd._lib.CDH_F64, cd._lib.CDH_WLS, n, 2 * n, 0, p, 0))   # half of a row-sharded problem
    assert call(h, cc=None) == BAD and b"row-sharded" in L.cdh_last_error(h)
    cd._lib.check(L.cdh_destroy(h))
    assert call(None) == BAD and b"NULL" in L.cdh_last_error(None)

    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    assert call(f._h) == cd._lib.CDH_OK
    good = (G.copy(), c.copy(), sw.copy())

    def bw(t, v):
        out = H.copy()
        out[t] = v
        return out

    for kw, word in ((dict(m=0), b"65536"), (dict(m=65537), b"65536"), (dict(bw=None), b"bandwidth"), (dict(z0=None), b"point 0"),
                     (dict(g=None), b"out_G"), (dict(ix=None), b"base_idx1"), (dict(bw=bw(2, 0.0)), b"point 2"),
                     (dict(bw=bw(3, -0.5)), b"point 3"), (dict(bw=bw(1, np.nan)), b"point 1"),
                     (dict(z0=np.array([0.2, 0.4, np.inf, 0.8])), b"point 2"), (dict(z0=np.array([np.nan, 0.4, 0.6, 0.8])), b"point 0"),
                     (dict(lo=np.array([-1, 7, -1, n], dtype=np.int64)), b"point 3"),
                     (dict(lo=np.array([-1, -2, -1, 0], dtype=np.int64)), b"point 1"), (dict(kind=2), b"kernel"),
                     (dict(wpow=0), b"wpow"), (dict(wpow=3), b"wpow"), (dict(mb=0), b"mb"),
                     (dict(mb=65, ix=np.ones(65, dtype=np.int64)), b"mb"), (dict(ix=np.array([1, 0, 3], dtype=np.int64)), b"p_base"),
                     (dict(ix=np.array([1, 4, 3], dtype=np.int64)), b"p_base")):
        G[:], c[:], sw[:] = -1.0, -1.0, -1.0
        assert call(f._h, **kw) == BAD, kw
        msg = L.cdh_last_error(f._h)
        assert word in msg and b"cdh_vc_gram_batch" in msg, (kw, msg)
        assert (G == -1.0).all() and (c == -1.0).all() and (sw == -1.0).all(), kw      # refused before anything was written
        assert call(f._h) == cd._lib.CDH_OK                              # the handle stays usable after every refusal ...
        assert _same(G, good[0]) and _same(c, good[1]) and _same(sw, good[2])    # ... and gives what it gave
    # a non-finite z0 is not an error where the point leaves a row out, and z0 may be NULL when every point does
    assert call(f._h, z0=np.array([Z0[0], np.nan, Z0[2], np.inf])) == cd._lib.CDH_OK and _same(G, good[0])
    assert call(f._h, z0=None, lo=np.array([0, 7, 3, n - 1], dtype=np.int64)) == cd._lib.CDH_OK
    k = cd.GaussianKernel
    for kw in (dict(base_cols=[]), dict(base_cols=[0, 3]), dict(base_cols=[-1]), dict(wpow=3), dict(leave_out=[0, n]),
               dict(leave_out=[-1, -2])):
        with pytest.raises(cd.ArgumentError):
            f.expanded_gram_batch(k, 0.3, [0.5, 0.6], **kw)
    for args in ((k, [0.3, -1.0], 0.5), (k, 0.3, [0.5, np.inf]), (k, 0.3, None), (k, 0.3, np.zeros(65537)), (7, 0.3, 0.5)):
        with pytest.raises(cd.ArgumentError):
            f.expanded_gram_batch(*args)
    with pytest.raises(TypeError):
        f.expanded_gram_batch("gaussian", 0.3, 0.5)
    with pytest.raises(cd.DimensionMismatch):
        f.expanded_gram_batch(k, [0.3, 0.4], [0.5, 0.6, 0.7])
    with pytest.raises(cd.DimensionMismatch):
        f.expanded_gram_batch(k, 0.3, 0.5, e=e[:-1])
    G1, c1, s1 = f.expanded_gram_batch(k, H, Z0, leave_out=LO)
    assert _same(G1, good[0].transpose(0, 2, 1)) and _same(c1, good[1]) and _same(s1, good[2])
    f.close()


# ---- 6. bit-identical ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [3001, 70001])
def test_two_calls_and_two_handles_agree_bit_for_bit(dtype, n):
    p, Q, m = 10, 2, 40
    X, z, y, e = _random_data(3, n, p, dtype)
    assert BP.plan(n, Q, p, m)["resident"] == (n == 3001)
    rng = np.random.default_rng(8)
    h, z0 = 0.2 + 0.2 * rng.random(m), rng.random(m)
    lo = np.where(np.arange(m) % 3 == 0, rng.integers(0, n, size=m), -1)
    outs = []
    for _ in range(2):
        f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
        a = f.expanded_gram_batch(cd.GaussianKernel, h, z0, leave_out=lo, wpow=2, e=e)
        b = f.expanded_gram_batch(cd.GaussianKernel, h, z0, leave_out=lo, wpow=2, e=e)
        assert all(_same(u, v) for u, v in zip(a, b))
        outs.append(a)
        f.close()
    assert all(_same(u, v) for u, v in zip(*outs))


# ---- 7. front ends ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [0, 1, 2])
def test_locpoly_on_a_grid_is_the_single_points_column_by_column(Q):
    from _vc_numpy import gen_data
    X, z, y = gen_data(np.random.default_rng(500), 500, 2, 0)
    zgrid = np.arange(0.01, 0.99, 0.2)
    assert zgrid.shape[0] == 5
    out = cd.locpoly(X, z, y, zgrid, Q, cd.EpanechnikovKernel(0.6))
    assert out.shape == (2 * (Q + 1), 5)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    for ind, z0 in enumerate(zgrid):
        assert _same(out[:, ind], cd.locpoly(f, None, None, float(z0), None, cd.EpanechnikovKernel(0.6))), (Q, ind)
    f.close()


def test_lvocv_locpoly_against_a_loop_over_the_single_point_export():
    """The routes share the Gram matrices bit for bit (section 1) and, asserted here, the coefficients: in this numpy the
    stacked solve runs LAPACK's solver block by block on the systems the per-point solve gives it.  They differ in the
    rounding of the p-term dot product X[i] . beta (einsum against @: at most (p + 1) u sum |x beta| each side) and of the
    running sum over the n observations."""
    from _vc_numpy import gen_data
    from coordinatedescent_jl_amd import api
    n, p, Q, hs = 60, 2, 1, [0.3, 0.5]
    Q1, u = Q + 1, 2.0 ** -53
    X, z, y = gen_data(np.random.default_rng(60), n, p, 0)
    assert X.shape == (n, p)
    mse = cd.lvocv_locpoly(X, z, y, Q, hs, cd.GaussianKernel)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    for ih, h in enumerate(hs):
        want, slack = 0.0, 0.0
        Gs, cs, hb = [], [], []
        for i in range(n):
            G, c, _ = f.expanded_gram(cd.GaussianKernel(h), leave_out=i)
            d = np.sqrt(np.diag(G))
            hbeta = np.linalg.solve(G / np.outer(d, d), c / d) / d
            yh = X[i] @ hbeta[::Q1]
            want += (yh - y[i]) ** 2
            slack += 2 * abs(yh - y[i]) * (p + 1) * u * np.abs(X[i] * hbeta[::Q1]).sum()
            Gs.append(G), cs.append(c), hb.append(hbeta)
        assert _same(api._solve_scaled_stack(np.stack(Gs), np.stack(cs)), np.stack(hb))      # the coefficients first: no difference
        bound = slack + n * u * want
        print(f"lvocv_locpoly h={h}: |batch - loop| = {abs(mse[ih] - want):.3e}, bound {bound:.3e}, MSE {want:.6f}")
        assert abs(mse[ih] - want) <= bound, (h, mse[ih], want, bound)
    assert np.array_equal(cd.lvocv_locpoly(f, None, None, None, hs, cd.GaussianKernel), mse)   # a resident loss serves as X
    f.close()


def test_split_locpoly_is_the_per_point_loop():
    """The parent's route restated: one cdh_vc_gram and one scaled solve per grid point, then the same interpolation loop."""
    from _vc_numpy import gen_data
    n, Q, hs = 120, 1, [0.3, 0.6]
    X, z, y = gen_data(np.random.default_rng(21), n, 2, 0)
    Xt, zt, yt = gen_data(np.random.default_rng(22), n, 2, 0)
    zt = 0.05 + 0.9 * zt
    zgrid = np.linspace(0.0, 1.0, 7)
    mse = cd.split_locpoly(X, z, y, Xt, zt, yt, zgrid, Q, hs, cd.GaussianKernel)
    f = cd.CDVaryingCoefficientLoss(y, X, z, Q)
    for ih, h in enumerate(hs):
        B = np.zeros((f.p, zgrid.shape[0]))
        for ind, z0 in enumerate(zgrid):
            G, c, _ = f.expanded_gram(cd.GaussianKernel(h), z0)
            d = np.sqrt(np.diag(G))
            B[:, ind] = np.linalg.solve(G / np.outer(d, d), c / d) / d
        want, bi = 0.0, np.zeros(f.p)
        for i in range(n):
            cd.get_beta_(bi, zgrid, B, zt[i])
            want += (float(yt[i]) - float(Xt[i, :] @ bi[::Q + 1])) ** 2
        assert mse[ih] == want, (h, mse[ih], want)
    f.close()
