"""cvLassoPath on the device against the CPU oracle and the numpy twin (tests/_cv_numpy.py), on one small problem whose
selection is interior (the twin on the oracle's paths gives index_min = 7 and index_1se = 6, with gaps in cvm near 3e-3):
every fold's path against O.LassoPath on the row subset, the errors against the twin evaluated on the device's own
coefficients within the forward bound of cdh_path_sse, the curve and the two rules, the full path against cd.LassoPath, and
the state a passed-in handle is left in -- also when a fold's solve raises."""
import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
import _cv_numpy as CV

pytestmark = pytest.mark.gpu

BETA_TOL = 1e-10           # the suite's (tests/_onchip_edge_cases.py, tests/_quad_cases.py)
F32_TOL = 1e-4             # fp32 storage: what test_fp32_against_fp64_oracle declares (absolute on beta, values O(1))
N, P, K, M = 601, 40, 3, 12


def _make():
    rng = np.random.default_rng(1)
    X = np.asfortranarray(rng.standard_normal((N, P)))
    bstar = np.zeros(P)
    bstar[:5] = (2.0, -1.5, 1.0, 0.5, -0.25)
    Y = X @ bstar + rng.standard_normal(N)
    folds = (rng.permutation(N) % K).astype(np.int32)
    lam = np.max(np.abs(X.T @ Y)) / N * np.geomspace(0.9, 0.005, M)
    return X, Y, folds, lam


X, Y, FOLDS, LAM = _make()
_ORACLE = {}


def _opts(mod, randomize):
    return mod.CDOptions(maxIter=5000, optTol=1e-12, randomize=randomize, seed=7)


def _oracle_fold_paths(ids, standardize, randomize):
    """O.LassoPath on the training rows of every fold; computed once per variant and never changed."""
    key = (ids.tobytes(), standardize, randomize)
    if key not in _ORACLE:
        out = []
        for k in range(K):
            tr = ids != k
            _, betas = O.LassoPath(np.asfortranarray(X[tr]), Y[tr], LAM, _opts(O, randomize), standardizeX=standardize)
            out.append(np.stack(betas, axis=1))
        _ORACLE[key] = out
    return _ORACLE[key]


def _check(res, ids, standardize, randomize, dtype=np.float64):
    tol = BETA_TOL if dtype == np.float64 else F32_TOL
    Xs, Ys = X.astype(dtype).astype(np.float64), Y.astype(dtype).astype(np.float64)      # the values as stored
    sizes = np.bincount(ids, minlength=K)
    np.testing.assert_array_equal(res.fold_sizes, sizes)
    np.testing.assert_array_equal(res.lambdapath, LAM)
    want = _oracle_fold_paths(ids, standardize, randomize)
    assert len(res.fold_paths) == K and res.fold_mse.shape == res.train_mse.shape == (K, M)
    for k in range(K):
        fp = res.fold_paths[k]
        assert fp.lambdapath == list(LAM) and len(fp.betapath) == M
        beta = np.stack([b.dense() for b in fp.betapath], axis=1)
        err = np.max(np.abs(beta - want[k]))
        print(f"fold {k}: max|beta - oracle| = {err:.3e}")
        np.testing.assert_allclose(beta, want[k], rtol=0, atol=tol)
        # the errors: the twin on the device's own coefficients, within the bound of the sums as cdh_path_sse takes them
        S = np.nonzero(np.any(beta != 0.0, axis=1))[0]
        s = max(len(S), 1)
        wh, wt, ah, at = CV.path_sse(Xs, Ys, ids, k, np.arange(1, P + 1), beta)
        nh, nt = sizes[k], N - sizes[k]
        assert np.all(np.abs(res.fold_mse[k] - wh / nh) <= CV.sse_bound(s, nh, ah) / nh)
        assert np.all(np.abs(res.train_mse[k] - wt / nt) <= CV.sse_bound(s, nt, at) / nt)
    cvm, cvsd = CV.cv_curve(sizes, res.fold_mse)
    np.testing.assert_allclose(res.cvm, cvm, rtol=1e-13)
    np.testing.assert_allclose(res.cvsd, cvsd, rtol=1e-13)
    assert (res.index_min, res.index_1se) == CV.select(LAM, cvm, cvsd) == (7, 6)
    assert res.lambda_min == LAM[7] and res.lambda_1se == LAM[6]
    # the full path is LassoPath's, bit for bit
    fresh = cd.CDLeastSquaresLoss(Y.astype(dtype), np.asfortranarray(X.astype(dtype)))
    ref = cd.LassoPath(fresh, None, LAM, _opts(cd, randomize), standardizeX=standardize)
    fresh.close()
    assert res.path.lambdapath == ref.lambdapath
    for a, b in zip(res.path.betapath, ref.betapath):
        np.testing.assert_array_equal(a.dense(), b.dense())
        assert a.nzval2ind.tolist() == b.nzval2ind.tolist()


@pytest.mark.parametrize("standardize", (True, False), ids=("std", "raw"))
def test_cv_against_the_oracle_and_the_twin(standardize):
    res = cd.cvLassoPath(X, Y, LAM, K=K, folds=FOLDS, options=_opts(cd, False), standardizeX=standardize, keep_fold_paths=True)
    _check(res, FOLDS, standardize, False)


def test_cv_with_ids_from_the_seed():
    ids = CV.fold_ids(N, K, 4)
    res = cd.cvLassoPath(X, Y, LAM, K=K, folds=None, seed=4, options=_opts(cd, False), keep_fold_paths=True)
    _check(res, ids, True, False)
    again = cd.cvLassoPath(X, Y, LAM, K=K, folds=ids, options=_opts(cd, False))
    np.testing.assert_array_equal(again.fold_mse, res.fold_mse)         # the same ids, whoever drew them: the same bits
    assert again.fold_paths is None and again.path is not None
    assert cd.cvLassoPath(X, Y, LAM, K=K, folds=ids, options=_opts(cd, False), full_path=False).path is None


def test_cv_with_shuffled_sweeps():
    res = cd.cvLassoPath(X, Y, LAM, K=K, folds=FOLDS, options=_opts(cd, True), keep_fold_paths=True)
    _check(res, FOLDS, True, True)


def test_cv_on_fp32_storage():
    f = cd.CDLeastSquaresLoss(Y.astype(np.float32), np.asfortranarray(X.astype(np.float32)))
    res = cd.cvLassoPath(f, None, LAM, K=K, folds=FOLDS, options=_opts(cd, False), keep_fold_paths=True)
    _check(res, FOLDS, True, False, dtype=np.float32)
    f.close()


def _is_plain_least_squares(f):
    """On CDH_LS (no weights to read), no folds (a held-out sum is refused), and lasso on it is lasso on a fresh handle."""
    with pytest.raises(cd.ArgumentError, match="no observation weights"):
        f.w
    with pytest.raises(cd.ArgumentError, match="cdh_set_folds first"):
        f.path_sse(0, [1], np.zeros((1, 1)))
    opts = cd.CDOptions(maxIter=2000, optTol=1e-10, randomize=False)
    got = cd.lasso(f, None, float(LAM[5]), options=opts)
    g = cd.CDLeastSquaresLoss(Y, X)
    want = cd.lasso(g, None, float(LAM[5]), options=opts)
    np.testing.assert_array_equal(got.x.dense(), want.x.dense())
    assert got.x.nzval2ind.tolist() == want.x.nzval2ind.tolist() and got.x.nnz >= 5
    np.testing.assert_array_equal(got.residuals, want.residuals)
    assert got.sigma == want.sigma and f.last_stats == g.last_stats
    g.close()


def test_a_passed_in_handle_comes_back_as_it_went_in():
    f = cd.CDLeastSquaresLoss(Y, X)
    x = cd.SparseIterate(P)
    cd.coordinateDescent_(x, f, cd.ProxL1(float(LAM[3])), _opts(cd, False))      # an iterate synced to it before the call
    mode = f.gradient_cache_mode()
    res = cd.cvLassoPath(f, None, LAM, K=K, folds=FOLDS, options=_opts(cd, False), full_path=False)
    assert (res.index_min, res.index_1se) == (7, 6) and f.gradient_cache_mode() == mode
    _is_plain_least_squares(f)
    f.close()


def test_a_passed_in_handle_comes_back_when_a_fold_raises():
    f = cd.CDLeastSquaresLoss(Y, X)
    with pytest.raises(TypeError):                       # the first fold's first solve cannot convert its options
        cd.cvLassoPath(f, None, LAM, K=K, folds=FOLDS, options=cd.CDOptions(maxIter=None))
    _is_plain_least_squares(f)
    f.close()
