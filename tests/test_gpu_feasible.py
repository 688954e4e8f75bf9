"""Penalty loadings on the device: k_col_loadings -> k_col_loadings_reduce behind cdh_loadings / getLoadings
(_getLoadings!, src/utils.jl:153-164), and the two front ends built on it and on the screening OLS: feasibleLasso_
(src/lasso.jl:154-194) and refitLassoPath (:208-225).

The kernel is checked the way tests/test_gpu_kernel_sums.py checks k_col_dots: on exactly summable integer data at every
edge of its indexing (named from the constants of tests/_sweep_plan.py, the twin of csrc/sweep_plan.hpp, and asserted to be reached), and on rounded data
against a bound written from the number of terms.  The front ends are checked against tests/_feasible_oracle.py, the
restatement of the reference on the CPU oracle, whose own checks are in tests/test_feasible_oracle.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
import _feasible_oracle as FO
import _sweep_plan as SP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53


K_BLOCK, K_COL_GROUP, K_COL_BATCH, K_COL_CHUNKS = SP.K_BLOCK, SP.K_COL_GROUP, SP.K_COL_BATCH, SP.K_COL_CHUNKS


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nv(dtype):
    return 2 if dtype == np.float64 else 4          # elements per 16-byte vector


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


_chunks = SP.col_dots_chunks      # the row chunks of each launch: col_loadings takes col_dots' batches and chunks


def _at_beta_zero(y, X):
    f = cd.CDLeastSquaresLoss(y, X)
    cd._lib.check(f._L.cdh_initialize(f._h, f.p, 0, None, None), f._h)     # beta = 0: r = y
    return f


def _exact(X, e):
    """(sum_i (x_ij e_i)^2 in long double, Gamma_j from it) of the data as stored."""
    t = X.astype(np.longdouble) * e.astype(np.longdouble)[:, None]
    S = np.sum(t * t, axis=0)
    return S, np.sqrt(S / np.longdouble(X.shape[0]))


def _gamma_bar(n):
    """Relative bar for Gamma_j.  Every term is non-negative, so any order of summing n terms, with the product and the fma
    of each, is within (n + 3) 2^-53 of S_j relatively; the square root halves that, and the division and the root add
    2 2^-53.  (The long-double yardstick's own error, 2^-64 per operation, is far below this.)"""
    return 0.5 * (n + 3) * U64 + 2 * U64


# ---- 1. exact sums ---------------------------------------------------------------------------------------------------------
def _row_case(case, dtype):
    nv, vb = _nv(dtype), K_BLOCK * _nv(dtype)
    return {"n1": 1, "vector_minus_1": nv - 1, "vector": nv, "vector_plus_1": nv + 1,
            "block_minus_1": vb - 1, "block": vb, "block_plus_1": vb + 1,
            "chunks_ragged": (2 * K_COL_CHUNKS * K_BLOCK + 777) * nv + 1}[case]


ROW_CASES = ["n1", "vector_minus_1", "vector", "vector_plus_1", "block_minus_1", "block", "block_plus_1", "chunks_ragged"]
COL_CASES = [1, 7, 8, 9, 4095, 4096, 4097]
DTYPES = [np.float64, np.float32]


def _integer_problem(n, p, dtype):
    rng = np.random.default_rng(1000 * p + n)
    X = (rng.integers(1, 4, size=(p, n)) * rng.choice([-1, 1], size=(p, n))).T.astype(dtype)   # Fortran order
    y = rng.integers(-4, 5, size=n).astype(dtype)
    assert 144 * n < 2 ** 53                           # every (x r)^2 <= 144 is an integer, and so is every partial sum
    return X, y


def _check_exact(n, p, dtype):
    X, y = _integer_problem(n, p, dtype)
    f = _at_beta_zero(y, X)
    t = X.astype(np.float64) * y.astype(np.float64)[:, None]
    S = np.sum(t * t, axis=0)
    np.testing.assert_array_equal(cd.getLoadings(f), np.sqrt(S / float(n)))
    f.close()


@pytest.mark.parametrize("case", ROW_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_loadings_are_exact_on_integer_data_at_every_row_edge(cus, dtype, case):
    n, p, nv = _row_case(case, dtype), 9, _nv(dtype)
    nvec = -(-n // nv)
    (chunks,) = _chunks(n, p, dtype, cus)
    reached = {"n1": n == 1,
               "vector_minus_1": nvec == 1 and n % nv == nv - 1,
               "vector": nvec == 1 and n % nv == 0,
               "vector_plus_1": nvec == 2 and n % nv == 1,
               "block_minus_1": nvec == K_BLOCK and n % nv == nv - 1 and chunks == 1,   # the last thread's vector is ragged
               "block": nvec == K_BLOCK and n % nv == 0 and chunks == 1,                # one block, every thread one vector
               "block_plus_1": nvec == K_BLOCK + 1 and chunks == 2,                     # a second chunk of one thread
               # every chunk's threads take several strides, the last stride is partial and ends inside a vector
               "chunks_ragged": chunks == K_COL_CHUNKS and nvec > 2 * chunks * K_BLOCK
                                and nvec % (chunks * K_BLOCK) != 0 and n % nv != 0}[case]
    assert reached, (case, n, nvec, chunks)
    _check_exact(n, p, dtype)


@pytest.mark.parametrize("p", COL_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_loadings_are_exact_on_integer_data_at_every_column_edge(cus, dtype, p):
    n = 67
    chunks = _chunks(n, p, dtype, cus)
    reached = {1: p < K_COL_GROUP, 7: p == K_COL_GROUP - 1, 8: p == K_COL_GROUP, 9: p == K_COL_GROUP + 1,
               4095: p == K_COL_BATCH - 1 and len(chunks) == 1 and p % K_COL_GROUP != 0,
               4096: p == K_COL_BATCH and len(chunks) == 1,
               4097: p == K_COL_BATCH + 1 and len(chunks) == 2}[p]     # a second batch of one column, written at an offset
    assert reached, (p, chunks)
    _check_exact(n, p, dtype)


# ---- 2. rounded data ----------------------------------------------------------------------------------------------------
def _normal_problem(n, p, dtype, seed=31):
    rng = np.random.default_rng(seed + n)
    return np.asfortranarray(rng.standard_normal((n, p)).astype(dtype)), rng.standard_normal(n).astype(dtype)


@pytest.mark.parametrize("n", [4099, 65537])
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_loadings_on_rounded_data_stay_within_the_term_count_bound(dtype, n):
    X, y = _normal_problem(n, 9, dtype)
    f = _at_beta_zero(y, X)
    got = cd.getLoadings(f)
    f.close()
    _, G = _exact(X, y)
    err = (np.abs(got - G) / G).astype(np.float64)
    print(f"loadings {np.dtype(dtype).name} n={n}: max rel err {err.max():.3e}, bar {_gamma_bar(n):.3e}")
    assert np.all(err <= _gamma_bar(n)), (err.max(), _gamma_bar(n))


def test_the_bound_has_teeth_one_row_is_a_hundred_bars():
    """At n = 4099 most single terms (x_ij r_i)^2 exceed 100 x the bar on their column's sum: a dropped or doubled row
    cannot pass the test above."""
    n = 4099
    X, y = _normal_problem(n, 9, np.float64)
    S, _ = _exact(X, y)
    t = (X * y[:, None]) ** 2
    assert np.mean(t > 100 * (n + 3) * U64 * S.astype(np.float64)) > 0.9


# ---- 3. stale residual --------------------------------------------------------------------------------------------------
def _assert_loadings_of_downloaded_r(f, X):
    got = cd.getLoadings(f)
    _, G = _exact(X, f.r)                              # (downloaded afterwards: the residual of the solve's own iterate)
    err = (np.abs(got - G) / G).astype(np.float64)
    assert np.all(err <= _gamma_bar(X.shape[0])), (err.max(), _gamma_bar(X.shape[0]))
    return got


def test_loadings_after_a_one_launch_solve_read_the_solves_residual(monkeypatch):
    monkeypatch.setenv("CDH_SMALL_PATH", "1")          # what a new handle does by default (tests/conftest.py turns it off)
    X, y, lam0 = FO.recipe(1)
    f, x = cd.CDLeastSquaresLoss(y, X), cd.SparseIterate(FO.P)
    before = cd.getLoadings(f)
    cd.coordinateDescent_(x, f, cd.ProxL1(lam0), cd.CDOptions(**FO.CD))
    assert f.onchip_stats()["solves"] == 1 and x.nnz > 0
    got = _assert_loadings_of_downloaded_r(f, X)
    assert np.max(np.abs(got - before) / before) > 1e-3    # (the residual before the solve would not have passed)
    np.testing.assert_allclose(f.r, y - X @ x.dense(), rtol=0, atol=1e-9)
    f.close()


def test_loadings_after_cache_served_solves_read_the_solves_residual():
    rng = np.random.default_rng(8)
    n, p = 3000, 400
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = X[:, :10] @ rng.standard_normal(10) + rng.standard_normal(n)
    f, x = cd.CDLeastSquaresLoss(y, X), cd.SparseIterate(p)
    f.set_onchip_solve(False)
    f.set_gradient_cache(3)
    opt = cd.CDOptions(maxIter=500, optTol=1e-12, randomize=False)
    for lam in (0.3, 0.15, 0.08):
        cd.coordinateDescent_(x, f, cd.ProxL1(lam), opt)
        before = cd.getLoadings(f) if lam == 0.3 else before
    assert f.device_loop_stats()["launches"] > 0 and f.cache_stats()["passes"] > 0
    got = _assert_loadings_of_downloaded_r(f, X)
    assert np.max(np.abs(got - before) / before) > 1e-3
    np.testing.assert_allclose(f.r, y - X @ x.dense(), rtol=0, atol=1e-9)
    f.close()


# ---- 4. read-only -------------------------------------------------------------------------------------------------------
def _state(f):
    beta = np.zeros(f.p)
    cd._lib.check(f._L.cdh_get_beta(f._h, _vp(beta)), f._h)
    return beta.tobytes(), f.X_cols(0, f.p).tobytes(), f.y.tobytes(), np.float64(cd.objective(f)).tobytes()


@pytest.mark.parametrize("route", ["streamed", "one_launch"])
def test_a_call_leaves_the_handle_as_it_found_it(monkeypatch, route):
    """Two handles through the same two solves, one of them asked for its loadings in between: same iterates, same pass and
    visit counts, same state.  (streamed: r is current throughout; one_launch: the call is what rebuilds the lazy r.)"""
    monkeypatch.setenv("CDH_SMALL_PATH", "1" if route == "one_launch" else "0")
    X, y, lam0 = FO.recipe(2)
    om = 0.5 + np.random.default_rng(5).random(FO.P)
    opt = cd.CDOptions(maxIter=2000, optTol=1e-9, randomize=False)
    out = []
    for query in (False, True):
        f, x = cd.CDLeastSquaresLoss(y, X), cd.SparseIterate(FO.P)
        cd.coordinateDescent_(x, f, cd.ProxL1(lam0, om), opt)
        if query:
            cd.getLoadings(f)
            cd.getLoadings(f)
        cd.coordinateDescent_(x, f, cd.ProxL1(0.5 * lam0, om), opt)
        out.append((x.dense().tobytes(), x.nzval2ind.tobytes(), f.last_stats["passes"], f.last_stats["visits"],
                    str(f.onchip_stats()), _state(f)))
        f.close()
    assert out[0] == out[1]


def test_a_call_between_cache_served_solves_changes_no_iterate_and_no_count():
    """The same with the gradient cache serving the solves: the call makes r catch up with the pending moves earlier than it
    otherwise would, and nothing the solves read (beta, the penalty, the cache's reference point, the dots) moves."""
    rng = np.random.default_rng(9)
    n, p = 3000, 400
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = X[:, :10] @ rng.standard_normal(10) + rng.standard_normal(n)
    opt = cd.CDOptions(maxIter=500, optTol=1e-12, randomize=False)
    out = []
    for query in (False, True):
        f, x = cd.CDLeastSquaresLoss(y, X), cd.SparseIterate(p)
        f.set_onchip_solve(False)
        f.set_gradient_cache(3)
        rec = []
        for lam in (0.3, 0.15, 0.08):
            cd.coordinateDescent_(x, f, cd.ProxL1(lam), opt)
            rec.append((x.dense().tobytes(), x.nzval2ind.tobytes(), f.last_stats["passes"], f.last_stats["visits"]))
            if query:
                cd.getLoadings(f)
        cs = f.cache_stats()
        out.append((rec, cs["passes"], cs["settled_visits"], cs["exact_visits"], cs["gram_columns"]))
        f.close()
    assert out[0] == out[1]


# ---- 5. bit-identical ----------------------------------------------------------------------------------------------------
def test_loadings_are_bit_identical_call_to_call_and_handle_to_handle():
    X, y = _normal_problem(65537, 9, np.float64)
    got = []
    for _ in range(2):
        f = _at_beta_zero(y, X)
        got += [cd.getLoadings(f).tobytes(), cd.getLoadings(f).tobytes()]
        f.close()
    assert len(set(got)) == 1


# ---- 6. feasibleLasso_ end to end -----------------------------------------------------------------------------------------
@pytest.fixture
def loadings_calls(monkeypatch):
    """Counts getLoadings as feasibleLasso_ calls it: one after the init, one per round."""
    calls, real = [], cd.api.getLoadings

    def counted(f):
        calls.append(1)
        return real(f)
    monkeypatch.setattr(cd.api, "getLoadings", counted)
    return calls


def _run(seed, init, dtype=np.float64, **kw):
    X, y, lam0 = FO.recipe(seed)
    f, x = cd.CDLeastSquaresLoss(y.astype(dtype), X.astype(dtype)), cd.SparseIterate(FO.P)
    o = cd.IterLassoOptions(initProcedure=init, optionsCD=cd.CDOptions(**FO.CD), **kw)
    return f, x, cd.feasibleLasso_(x, f, None, lam0, o), lam0


@pytest.mark.parametrize("init", FO.INITS)
@pytest.mark.parametrize("seed", FO.SEEDS)
def test_feasible_lasso_matches_the_restatement(loadings_calls, seed, init):
    want = FO.solved(seed, init)
    assert all(abs(s - FO.OPT_TOL) > 0.05 * FO.OPT_TOL for s in want.stats)      # (the input condition, from the oracle alone)
    f, x, sol, lam0 = _run(seed, init)
    rounds = len(loadings_calls) - 1
    print(f"feasibleLasso_ seed {seed} {init}: rounds {rounds} (oracle {len(want.stats)}), "
          f"max|beta - oracle| {np.max(np.abs(x.dense() - want.x.dense())):.3e}, sigma {sol.sigma} (oracle {want.sigma})")
    assert rounds == len(want.stats)
    np.testing.assert_allclose(x.dense(), want.x.dense(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(sol.sigma, want.sigma, rtol=1e-6)
    assert sol.x is x and sol.penalty.lambda0 == lam0
    assert sol.penalty.lam.tobytes() == cd.getLoadings(f).tobytes()             # the loadings AFTER the last solve (the aliasing)
    f.close()


def test_feasible_lasso_on_fp32_storage(loadings_calls):
    want = FO.solved(1, "Screening")
    f, x, sol, _ = _run(1, "Screening", dtype=np.float32)
    assert len(loadings_calls) - 1 == len(want.stats)
    np.testing.assert_allclose(x.dense(), want.x.dense(), rtol=0, atol=3e-4)
    f.close()


def test_feasible_lasso_returns_after_maxiter_rounds(loadings_calls):
    want = FO.solved(1, "Screening", maxIter=2)
    assert len(want.stats) == 2 and want.stats[-1] >= FO.OPT_TOL
    f, x, sol, _ = _run(1, "Screening", maxIter=2)
    assert len(loadings_calls) - 1 == 2
    np.testing.assert_allclose(x.dense(), want.x.dense(), rtol=0, atol=1e-6)
    f.close()


def test_feasible_lasso_takes_host_arrays_like_the_other_front_ends():
    X, y, lam0 = FO.recipe(3)
    x = cd.SparseIterate(FO.P)
    sol = cd.feasibleLasso_(x, X, y, lam0, cd.IterLassoOptions(initProcedure="WarmStart", optionsCD=cd.CDOptions(**FO.CD)))
    np.testing.assert_allclose(sol.x.dense(), FO.solved(3, "WarmStart").x.dense(), rtol=0, atol=1e-6)


def test_feasible_lasso_refuses_what_scaled_lasso_refuses():
    X, y, lam0 = FO.recipe(1)
    f = cd.CDLeastSquaresLoss(y, X)
    with pytest.raises(cd.ArgumentError, match="Incorrect initialization Symbol"):
        cd.feasibleLasso_(cd.SparseIterate(FO.P), f, None, lam0, cd.IterLassoOptions(initProcedure="Oracle"))
    for init in FO.INITS:
        o = cd.IterLassoOptions(initProcedure=init)
        raised = []
        for call in (lambda: cd.scaledLasso_(cd.SparseIterate(FO.P + 1), f, None, lam0, np.ones(FO.P), o),
                     lambda: cd.feasibleLasso_(cd.SparseIterate(FO.P + 1), f, None, lam0, o)):
            with pytest.raises(cd.DimensionMismatch) as e:
                call()
            raised.append(e.type)
        assert raised[0] is raised[1]
    x = cd.SparseIterate(FO.P)                          # the handle is still good
    cd.coordinateDescent_(x, f, cd.ProxL1(lam0), cd.CDOptions(**FO.CD))
    assert x.nnz > 0
    f.close()


# ---- 7. refitLassoPath ----------------------------------------------------------------------------------------------------
def test_refit_lasso_path_is_lstsq_on_every_distinct_support():
    X, y, _ = FO.recipe(1)
    lmax = float(np.max(np.abs(X.T @ y) / FO.N / O.stdX(X)))
    lams = [f * lmax for f in (1.05, 0.6, 0.3, 0.27, 0.1, 0.03)]
    opt = cd.CDOptions(maxIter=5000, optTol=1e-10, randomize=False)
    f = cd.CDLeastSquaresLoss(y, X)
    path = cd.LassoPath(f, None, lams, opt)
    sups = [tuple(sorted(int(k) for k in b.nzval2ind)) for b in path.betapath]
    assert len(sups) == 6 and sups[0] == () and any(a == b and a for a, b in zip(sups, sups[1:]))   # from the path itself
    assert 2 < len(set(sups)) < 6
    out = cd.refitLassoPath(path, X, y)
    assert sorted(out) == sorted(set(sups))
    for S, coef in out.items():
        assert coef.dtype == np.float64 and coef.shape == (len(S),)
        if S:
            want = np.linalg.lstsq(X[:, np.array(S) - 1], y, rcond=None)[0]
            np.testing.assert_allclose(coef, want, rtol=1e-9, atol=1e-12)
    assert out[()].shape == (0,)
    # a resident loss as X: the same dict, and the handle is left at beta = 0 with r = y
    out2 = cd.refitLassoPath(path, f, None)
    assert sorted(out2) == sorted(out) and all(out2[S].tobytes() == out[S].tobytes() for S in out)
    beta = np.ones(FO.P)
    cd._lib.check(f._L.cdh_get_beta(f._h, _vp(beta)), f._h)
    assert not beta.any() and f.r.tobytes() == y.tobytes() and f._synced is None
    f.close()


def test_refit_lasso_path_refuses_a_support_beyond_the_gram_limit():
    rng = np.random.default_rng(3)
    n, p = 8, 4100
    f = cd.CDLeastSquaresLoss(rng.standard_normal(n), np.asfortranarray(rng.standard_normal((n, p))))
    path = cd.LassoPathResult([0.1], [cd.SparseIterate(p, np.ones(p))])
    with pytest.raises(cd.ArgumentError):
        cd.refitLassoPath(path, f, None)
    f.close()


# ---- 8. row shards ----------------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_loadings_and_feasible_lasso_on_two_row_shards_over_the_host_exchange():
    a = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(ROOT, "tests", "feasible_shard_worker.py")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert a.returncode == 0, (a.stdout[-1500:], a.stderr[-3000:])
    assert "FEASIBLE_SHARDS_OK" in a.stdout


# ---- 9. ABI refusals -----------------------------------------------------------------------------------------------------
def test_cdh_loadings_refuses_null_arguments_and_leaves_the_handle_usable():
    X, y = _integer_problem(67, 9, np.float64)
    f = _at_beta_zero(y, X)
    out = np.zeros(9)
    assert f._L.cdh_loadings(None, _vp(out)) == cd._lib.CDH_BAD_ARG
    assert f._L.cdh_loadings(f._h, None) == cd._lib.CDH_BAD_ARG
    with pytest.raises(cd.ArgumentError):
        cd._lib.check(f._L.cdh_loadings(f._h, None), f._h)
    t = X * y[:, None]
    np.testing.assert_array_equal(cd.getLoadings(f), np.sqrt(np.sum(t * t, axis=0) / 67.0))
    f.close()
