"""The three exports under cvLassoPath on the device: cdh_set_folds, cdh_set_fold_weights (k_fold_weights) and cdh_path_sse
(k_path_sse -> k_gram_reduce).  The fold weights are compared value for value and through a solve against uploaded weights;
the sums on exactly summable integer data at every edge of the kernel's indexing (row tile, grid wrap, column groups, the
unrolled column loop), on rounded data against the forward bound of the sums as computed, for repeatability, and for leaving
a handle in the middle of a cache-served path exactly as it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cv_numpy as CV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = open(os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc", "cv_plan.hpp")).read()


def _constant(name):
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, PLAN).group(1))


G, ROWS, MAX_GRID = _constant("kCvGroup"), _constant("kCvRows"), _constant("kCvMaxGrid")
NS = (1, 2, 63, 64, 65, 4099, 65537)
WRAP = ROWS * MAX_GRID                                   # the first n whose tiles outnumber the grid is WRAP + 1
NS_SSE = NS + (ROWS - 1, ROWS, ROWS + 1, WRAP - 1, WRAP, WRAP + 1)
DTYPES = (np.float64, np.float32)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _folds(rng, n, K):
    ids = rng.permutation(n) % K                         # every fold non-empty for K <= n
    return ids.astype(np.int32)


def _wls(n, p, dtype, rng):
    X = np.asfortranarray(rng.integers(-2, 3, size=(n, p)).astype(dtype))
    y = rng.integers(-2, 3, size=n).astype(dtype)
    return cd.CDWeightedLSLoss(y, X, np.full(n, 0.5, dtype=dtype)), X, y


# ---- fold weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("n", NS)
def test_fold_weights_are_the_indicator(n, dtype):
    rng = np.random.default_rng(n)
    f, _, _ = _wls(n, 2, dtype, rng)
    f.set_fold_weights(-1)                               # no folds needed for all ones
    np.testing.assert_array_equal(f.w, np.ones(n, dtype=dtype))
    for K in (2, 3, 255):
        if K > n:
            with pytest.raises(cd.ArgumentError, match="K <= n"):
                f.set_folds(np.zeros(n, dtype=np.int32), K)
            continue
        ids = _folds(rng, n, K)
        np.testing.assert_array_equal(f.set_folds(ids, K), np.bincount(ids, minlength=K))
        for k in (0, K - 1, -1):
            f.set_fold_weights(k)
            w = f.w
            assert w.dtype == dtype
            np.testing.assert_array_equal(w, (ids != k).astype(dtype))
    f.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("start", ("wls", "ls"))
def test_a_solve_on_fold_weights_is_the_solve_on_uploaded_weights(dtype, start):
    rng = np.random.default_rng(5)
    n, p, K, k = 4099, 24, 3, 1
    X = np.asfortranarray(rng.standard_normal((n, p)).astype(dtype))
    y = (X[:, :4] @ np.array([2.0, -1.0, 0.5, 0.25]) + rng.standard_normal(n)).astype(dtype)
    ids = _folds(rng, n, K)
    w = (ids != k).astype(dtype)
    if start == "wls":
        f = cd.CDWeightedLSLoss(y, X, np.ones(n, dtype=dtype))
    else:                                                # a least-squares handle switched over, as cvLassoPath does
        f = cd.CDLeastSquaresLoss(y, X)
        cd.lasso(f, None, 0.3, options=cd.CDOptions(randomize=False))
        cd.check(f._L.cdh_set_loss(f._h, cd.CDH_WLS), f._h)
    f.set_folds(ids, K)
    f.set_fold_weights(k)
    g = cd.CDWeightedLSLoss(y, X, w)
    np.testing.assert_array_equal(cd.stdX(f, weighted=True), cd.stdX(g, weighted=True))
    opts = cd.CDOptions(maxIter=2000, optTol=1e-10, randomize=False)
    xf, xg = cd.SparseIterate(p), cd.SparseIterate(p)
    for lam in (0.2, 0.05, 0.01):                        # warm-started, as a path is
        om = cd.stdX(g, weighted=True)
        cd.coordinateDescent_(xf, f, cd.ProxL1(lam, om), opts)
        cd.coordinateDescent_(xg, g, cd.ProxL1(lam, om), opts)
        np.testing.assert_array_equal(xf.dense(), xg.dense())
        assert xf.nzval2ind.tolist() == xg.nzval2ind.tolist() and xf.nnz > 0
        assert f.last_stats["passes"] == g.last_stats["passes"] and f.last_stats["converged"]
    np.testing.assert_array_equal(f.r, g.r)
    f.close(), g.close()


def test_refusals_of_the_fold_exports():
    rng = np.random.default_rng(1)
    n = 40
    f, X, y = _wls(n, 2, np.float64, rng)
    ids = _folds(rng, n, 4)
    with pytest.raises(cd.ArgumentError, match="cdh_set_folds first"):
        f.set_fold_weights(0)                            # no folds
    for K in (1, 256):
        with pytest.raises(cd.ArgumentError, match="2 <= K <= 255"):
            f.set_folds(np.zeros(n, dtype=np.int32), K)
    with pytest.raises(cd.ArgumentError, match="fold 4 is empty"):
        f.set_folds(ids, 5)
    with pytest.raises(cd.ArgumentError, match="outside 0 .. K - 1"):
        f.set_folds(ids, 3)
    f.set_folds(ids, 4)
    with pytest.raises(cd.ArgumentError, match="below the K"):
        f.set_fold_weights(4)
    with pytest.raises(cd.ArgumentError):
        f.set_fold_weights(-2)
    np.testing.assert_array_equal(f.w, np.full(n, 0.5))  # every refusal left the weights alone
    f.set_folds(None, 0)                                 # dropped: fold weights need them again
    with pytest.raises(cd.ArgumentError, match="cdh_set_folds first"):
        f.set_fold_weights(0)
    f.close()
    ls = cd.CDLeastSquaresLoss(y, X)
    ls.set_folds(ids, 4)                                 # folds are not tied to a loss kind ...
    with pytest.raises(cd.ArgumentError, match="observation weights need the CDH_WLS loss"):
        ls.set_fold_weights(0)                           # ... the weights are
    ls.close()
    shard = cd.CDWeightedLSLoss(y, X, np.ones(n), n_total=2 * n, row_offset=0)
    for call in (lambda: shard.set_folds(ids, 4), lambda: shard.set_fold_weights(-1),
                 lambda: shard.path_sse(-1, [1], np.zeros((1, 1)))):
        with pytest.raises(cd.ArgumentError, match="row-sharded"):
            call()
    shard.close()


# ---- exact sums -------------------------------------------------------------------------------------------------------------------
def _exact(X, y, ids, k, idx1, B):
    """int64 sums of the integer-valued data (the products go through float64 BLAS, exactly: every value is a small integer)."""
    res = (y.astype(np.float64)[:, None] - X[:, idx1 - 1].astype(np.float64) @ B).astype(np.int64)
    sq = res * res
    held = (ids == k) if k >= 0 else np.zeros(len(y), dtype=bool)
    return sq[held].sum(axis=0), sq[~held].sum(axis=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("n", NS_SSE)
def test_path_sse_exact_on_integers(n, dtype):
    rng = np.random.default_rng(n + 7)
    p = 11
    f, X, y = _wls(n, p, dtype, rng)
    K = 3 if n >= 3 else (2 if n >= 2 else 0)
    ids = _folds(rng, n, K) if K else np.zeros(n, dtype=np.int32)
    if K:
        f.set_folds(ids, K)
    # Up to n = 4099 the full s x m set runs.  Beyond it (65537 and the three sizes at the grid wrap) the int64 reference is
    # what takes the time, so a picked set runs that still has every m and every s of the list once; the size just past the
    # wrap adds the three widths that differ in their number of groups.
    small = n <= 4099
    shapes = ([(s, m) for s in (1, 2, 63, 64, 65, 130) for m in (1, G - 1, G, G + 1, 2 * G + 1)] if small
              else [(1, 1), (2, G + 1), (63, G - 1), (64, G), (65, 2 * G + 1), (130, G)])
    if n == WRAP + 1:
        shapes += [(2, 1), (2, 2 * G + 1), (1, G + 1)]
    seen_repeat = False
    for s, m in shapes:
        idx1 = rng.integers(1, p + 1, size=s).astype(np.int64)          # s > p: coordinates repeat, their terms add
        seen_repeat |= len(set(idx1.tolist())) < s
        B = np.asfortranarray(rng.integers(-2, 3, size=(s, m)).astype(np.float64))
        for k in ((0, K - 1, -1) if K else (-1,)):
            want_h, want_t = _exact(X, y, ids, k, idx1, B)
            held, train = f.path_sse(k, idx1, B)
            np.testing.assert_array_equal(held.astype(np.int64), want_h, err_msg=str((s, m, k)))
            np.testing.assert_array_equal(train.astype(np.int64), want_t, err_msg=str((s, m, k)))
            assert np.all(held == np.floor(held)) and np.all(train == np.floor(train))
    assert seen_repeat
    # ldb > s, and either out pointer NULL
    s, m, ldb = 5, G + 1, 9
    idx1 = np.array([3, 3, 1, p, 2], dtype=np.int64)
    big = np.asfortranarray(rng.integers(-2, 3, size=(ldb, m)).astype(np.float64))
    k = 0 if K else -1
    want_h, want_t = _exact(X, y, ids, k, idx1, big[:s])
    oh, ot = np.zeros(m), np.zeros(m)
    cd.check(f._L.cdh_path_sse(f._h, k, s, _vp(idx1), m, _vp(big), ldb, _vp(oh), _vp(ot)), f._h)
    np.testing.assert_array_equal(oh.astype(np.int64), want_h)
    np.testing.assert_array_equal(ot.astype(np.int64), want_t)
    only_h, none = f.path_sse(k, idx1, big[:s], train=False)
    none2, only_t = f.path_sse(k, idx1, big[:s], held=False)
    assert none is None and none2 is None
    np.testing.assert_array_equal(only_h, oh)
    np.testing.assert_array_equal(only_t, ot)
    np.testing.assert_array_equal(f.w, np.full(n, 0.5, dtype=dtype))    # (and the weights were never touched)
    f.close()


# ---- rounded data against the forward bound ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(11)
    n, p, s, m, K = 4099, 50, 37, 2 * G + 1, 4
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = rng.standard_normal(n)
    ids = _folds(rng, n, K)
    idx1 = (rng.permutation(p)[:s] + 1).astype(np.int64)
    B = np.asfortranarray(rng.standard_normal((s, m)) * (rng.random((s, m)) < 0.4))
    return n, p, s, m, K, X, y, ids, idx1, B


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_path_sse_random_within_the_forward_bound(random_case, dtype):
    n, p, s, m, K, X, y, ids, idx1, B = random_case
    Xs, ys = np.asfortranarray(X.astype(dtype)), y.astype(dtype)        # the twin sees the values as stored
    f = cd.CDLeastSquaresLoss(ys, Xs)                                   # any loss kind may call it
    f.set_folds(ids, K)
    for k in (0, K - 1, -1):
        held, train = f.path_sse(k, idx1, B)
        again = f.path_sse(k, idx1, B)
        np.testing.assert_array_equal(again[0], held)                   # bit-identical run to run
        np.testing.assert_array_equal(again[1], train)
        wh, wt, ah, at = CV.path_sse(Xs, ys, ids, k, idx1, B)
        n_h = int(np.sum(ids == k)) if k >= 0 else 0
        eh, et = np.abs(held - wh), np.abs(train - wt)
        bh, bt = CV.sse_bound(s, n_h, ah), CV.sse_bound(s, n - n_h, at)
        print(f"k={k} {np.dtype(dtype).name}: max err/bound held {np.max(eh / np.maximum(bh, 1e-300)):.3f} "
              f"train {np.max(et / bt):.3f}")
        assert np.all(eh <= bh) and np.all(et <= bt)
        if k < 0:
            assert np.all(held == 0.0)
    f.close()


# ---- read-only, in the middle of a cache-served path ------------------------------------------------------------------------------
def _beta_and_support(f):
    beta, idx, nnz = np.zeros(f.p), np.zeros(f.p, dtype=np.int64), C.c_int64()
    cd.check(f._L.cdh_get_beta(f._h, _vp(beta)), f._h)
    cd.check(f._L.cdh_get_support(f._h, _vp(idx), C.byref(nnz)), f._h)
    return beta, idx[: nnz.value].tolist()


def test_path_sse_leaves_a_cache_served_path_as_it_was():
    rng = np.random.default_rng(3)
    n, p, s = 3000, 400, 10
    X = np.asfortranarray(rng.standard_normal((n, p)))
    Y = X[:, :s] @ rng.standard_normal(s) + rng.standard_normal(n)
    lams = np.exp(np.linspace(np.log(0.3), np.log(0.03), 8))
    opts = cd.CDOptions(maxIter=500, optTol=1e-12, randomize=False)
    ids = _folds(rng, n, 5)
    runs = []
    for probe in (True, False):
        f = cd.CDLeastSquaresLoss(Y, X)
        f.set_gradient_cache(2)
        cd.check(f._L.cdh_set_reuse_residual(f._h, 1), f._h)
        x, betas = cd.SparseIterate(p), []
        for i, lam in enumerate(lams):
            cd.coordinateDescent_(x, f, cd.ProxL1(lam), opts)
            betas.append((x.dense(), x.nzval2ind.tolist(), f.last_stats["passes"]))
            if probe and i == 3:
                before = (f.cache_stats(), f.cache_drift()["measured"], *_beta_and_support(f))
                assert before[0]["passes"] > 0                                                 # the cache is serving
                f.set_folds(ids, 5)
                S = np.array(x.nzval2ind, dtype=np.int64)
                held, train = f.path_sse(2, S, x.dense()[S - 1][:, None])
                after = (f.cache_stats(), f.cache_drift()["measured"], *_beta_and_support(f))
                assert before[0] == after[0] and before[1] == after[1]
                np.testing.assert_array_equal(before[2], after[2])
                assert before[3] == after[3]
                res = Y - X @ x.dense()
                np.testing.assert_allclose(held[0], np.sum(res[ids == 2] ** 2), rtol=1e-12)
                np.testing.assert_allclose(train[0], np.sum(res[ids != 2] ** 2), rtol=1e-12)
        runs.append((betas, f.cache_stats(), f.r))
        f.close()
    for (b1, sup1, p1), (b2, sup2, p2) in zip(runs[0][0], runs[1][0]):
        np.testing.assert_array_equal(b1, b2)
        assert sup1 == sup2 and p1 == p2
    assert runs[0][1] == runs[1][1]
    np.testing.assert_array_equal(runs[0][2], runs[1][2])


def test_refusals_of_path_sse():
    rng = np.random.default_rng(2)
    n, p = 50, 6
    f, X, y = _wls(n, p, np.float64, rng)
    L, h = f._L, f._h
    idx1, B, out = np.array([1, 2, 3], dtype=np.int64), np.zeros((3, 2), order="F"), np.zeros(2)
    big_idx, wide = np.ones(4097, dtype=np.int64), np.zeros((1, 1025), order="F")

    def refused(match, *args):
        assert L.cdh_path_sse(h, *args) == cd._lib.CDH_BAD_ARG
        assert re.search(match, L.cdh_last_error(h).decode()), L.cdh_last_error(h)

    refused("1 <= s <= 4096", -1, 0, _vp(idx1), 2, _vp(B), 3, _vp(out), None)
    refused("1 <= s <= 4096", -1, 4097, _vp(big_idx), 1, _vp(np.zeros((4097, 1))), 4097, _vp(out), None)
    refused("1 <= m <= 1024", -1, 3, _vp(idx1), 0, _vp(B), 3, _vp(out), None)
    refused("1 <= m <= 1024", -1, 1, _vp(idx1), 1025, _vp(wide), 1, _vp(np.zeros(1025)), None)
    refused("ldb", -1, 3, _vp(idx1), 2, _vp(B), 2, _vp(out), None)
    refused("idx1", -1, 3, _vp(np.array([1, 0, 3], dtype=np.int64)), 2, _vp(B), 3, _vp(out), None)
    refused("idx1", -1, 3, _vp(np.array([1, p + 1, 3], dtype=np.int64)), 2, _vp(B), 3, _vp(out), None)
    refused("both NULL", -1, 3, _vp(idx1), 2, _vp(B), 3, None, None)
    refused("cdh_set_folds first", 0, 3, _vp(idx1), 2, _vp(B), 3, _vp(out), None)
    refused("NULL", -1, 3, None, 2, _vp(B), 3, _vp(out), None)
    refused("NULL", -1, 3, _vp(idx1), 2, None, 3, _vp(out), None)
    f.set_folds(_folds(rng, n, 2), 2)
    refused("below the K", 2, 3, _vp(idx1), 2, _vp(B), 3, _vp(out), None)
    assert L.cdh_path_sse(h, 1, 3, _vp(idx1), 2, _vp(B), 3, _vp(out), None) == cd._lib.CDH_OK
    f.close()
    raw = cd.CDLeastSquaresLoss.__new__(cd.CDLeastSquaresLoss)
    raw._create(np.float64, n, p, 0, None, 0)                          # a handle that was only created has no y
    assert raw._L.cdh_path_sse(raw._h, -1, 3, _vp(idx1), 2, _vp(B), 3, _vp(out), None) == cd._lib.CDH_BAD_ARG
    assert b"cdh_set_y" in raw._L.cdh_last_error(raw._h)
    raw.close()
