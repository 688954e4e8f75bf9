"""CDQuadraticLoss (src/cd_differentiable_function.jl:299-348) on the device: single problems and batches that share A,
solved by k_quad_solve (csrc/quad_solve.hpp) with one workgroup per problem.

Parity bar, against the oracle's per-coordinate sweep of the same problem: beta within 1e-10, the SAME
passes, full passes, visits and convergence flag, and the same support ORDER (nzval2ind), ordered and shuffled.
A = X'X / n of a Gaussian X with n = 2p + 2 rows: positive diagonal, well conditioned (tests/_quad_cases.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
from _quad_cases import BETA_TOL, _A, _b, _same

pytestmark = pytest.mark.gpu

PMAX = cd.CDH_QUAD_MAX_P
OPT = dict(maxIter=20000, optTol=1e-12)


# ---- 1. the reference's known answer (test/coordinate_descent.jl:13-25) ------------------------------------------------------
def test_known_answer():
    f = cd.CDQuadraticLoss(np.eye(2), -np.array([1.0, 1.5]))
    x = cd.SparseIterate(2)
    cd.coordinateDescent_(x, f, cd.ProxL1(1.2), cd.CDOptions(randomize=False, warmStart=True))
    np.testing.assert_allclose(x.dense(), [0.0, 0.3], rtol=0, atol=1e-15)
    assert f.last_stats["converged"]
    f.close()


# ---- 2. single problems --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_pair(p):
    A, b = _A(p), _b(p, 0)
    return cd.CDQuadraticLoss(A, b), O.CDQuadraticLoss(A, b), b


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "omega"])
@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("rand", [False, True], ids=["ordered", "shuffled"])
@pytest.mark.parametrize("p", [1, 2, 63, 64, 65, 200, 1024, PMAX])
def test_single_problem_parity(p, rand, warm, weighted):
    f, fo, b = _loss_pair(p)
    rng = np.random.default_rng(31 * p + 4 * rand + 2 * warm + weighted)
    om = rng.random(p) + 0.5 if weighted else None
    score = np.abs(b) / (om if weighted else 1.0)
    if p >= 1024:
        lam = float(np.sort(score)[-31])                 # at most 30 coordinates clear the threshold from zero
    else:
        lam = 0.3 * float(score.max())
    x0 = np.where(rng.random(p) < 0.6, rng.random(p), 0.0) if warm else None
    x, xo = cd.SparseIterate(p, x0), O.SparseIterate(p, x0)
    o = dict(OPT, warmStart=warm, randomize=rand, seed=3, numSteps=50)
    cd.coordinateDescent_(x, f, cd.ProxL1(lam, om), cd.CDOptions(**o))
    st = O.coordinateDescent_(xo, fo, O.ProxL1(lam, om), O.CDOptions(**o))
    assert st["converged"]
    if p >= 1024:
        assert xo.nnz <= 30
    _same(f.last_stats, x, st, xo)
    if not warm:
        np.testing.assert_allclose(f.last_stats["lambda_max"], score.max(), rtol=1e-15)
    # the gradient the kernel carried is the gradient of where it ended
    np.testing.assert_allclose(f._gradient_vector(0), _A(p) @ x.dense() + b, rtol=0, atol=1e-11 * max(1.0, np.abs(b).max()))


# ---- 3. batches: every workgroup finds its own problem ---------------------------------------------------------------------
P_B, MAX_BATCH = 40, 320


def _batch_case(m, seed):
    rng = np.random.default_rng(100 + seed)
    B = np.stack([_b(P_B, 50 * seed + j, s=1 + j % 9) for j in range(m)], axis=1)
    lams = np.array([(0.05 + 0.6 * rng.random()) * np.abs(B[:, j]).max() for j in range(m)])
    return B, lams


def _check_batch(B, lams, opts, expect=None):
    A, m = _A(P_B), B.shape[1]
    f = cd.CDQuadraticLoss(A, B, max_batch=MAX_BATCH)
    xs = [cd.SparseIterate(P_B) for _ in range(m)]
    cd.coordinateDescent_(xs, f, [cd.ProxL1(l) for l in lams], cd.CDOptions(**opts))
    assert isinstance(f.last_stats, list) and len(f.last_stats) == m
    alone = cd.CDQuadraticLoss(A, B[:, :1], max_batch=1)
    for j in range(m):
        fo, xo = O.CDQuadraticLoss(A, B[:, j].copy()), O.SparseIterate(P_B)
        st = O.coordinateDescent_(xo, fo, O.ProxL1(lams[j]), O.CDOptions(**opts))
        _same(f.last_stats[j], xs[j], st, xo, tag=j)
        if expect:
            expect(j, st, xo)
        # the same problem as a batch of one: same kernel, deterministic -> the same bits
        alone.set_b(B[:, [j]])
        x1 = [cd.SparseIterate(P_B)]
        cd.coordinateDescent_(x1, alone, cd.ProxL1(lams[j]), cd.CDOptions(**opts))
        assert np.array_equal(x1[0].dense(), xs[j].dense()) and x1[0].nzval2ind.tolist() == xs[j].nzval2ind.tolist(), j
        assert alone.last_stats[0] == f.last_stats[j], j
    f.close()
    alone.close()


@pytest.mark.parametrize("m", [1, 2, 64, 300, MAX_BATCH])
def test_batch_indexing(m):
    B, lams = _batch_case(m, m)
    _check_batch(B, lams, dict(OPT, warmStart=True, randomize=(m % 2 == 0), seed=3))


def test_batch_workgroups_leave_at_different_times():
    B, lams = _batch_case(6, 9)
    lams[0] = 1.5 * np.abs(B[:, 0]).max()                # above its lambda_max: the solution is zero, found at once
    lams[1] = 1e-4 * np.abs(B[:, 1]).max()               # dense
    lams[2] = 1e-3 * np.abs(B[:, 2]).max()               # dense too: still moving when maxIter cuts it off
    seen = {}

    def expect(j, st, xo):
        seen[j] = (st["converged"], st["passes"], xo.nnz)

    _check_batch(B, lams, dict(maxIter=3, optTol=1e-12, warmStart=True, randomize=False, seed=3), expect)
    assert seen[0][0] and seen[0][2] == 0 and seen[0][1] < 3
    assert not seen[1][0] and seen[1][1] == 3 and seen[1][2] >= P_B // 2
    assert not seen[2][0] and seen[2][1] == 3
    assert len({v[1] for v in seen.values()}) > 1        # the workgroups did stop after different numbers of passes


# ---- 4. a penalty per problem: neighbourhood selection ----------------------------------------------------------------------
def test_per_problem_omega_neighbourhood_selection():
    p = 65
    A = _A(p)
    B = -A.copy()
    om = np.ones((p, p))
    om[np.diag_indices(p)] = np.inf
    lam = 0.08
    f = cd.CDQuadraticLoss(A, B)
    xs = [cd.SparseIterate(p) for _ in range(p)]
    o = dict(OPT, warmStart=True, randomize=True, seed=3)
    cd.coordinateDescent_(xs, f, [cd.ProxL1(lam, om[:, j]) for j in range(p)], cd.CDOptions(**o))
    nnz = 0
    for j in range(p):
        assert xs[j][j + 1] == 0.0 and (j + 1) not in xs[j].nzval2ind.tolist()
        fo, xo = O.CDQuadraticLoss(A, B[:, j].copy()), O.SparseIterate(p)
        st = O.coordinateDescent_(xo, fo, O.ProxL1(lam, om[:, j]), O.CDOptions(**o))
        _same(f.last_stats[j], xs[j], st, xo, tag=j)
        nnz += xo.nnz
    assert nnz > p                                       # (the problems are not all trivially zero)
    f.close()


# ---- 5. the plug-in interface ------------------------------------------------------------------------------------------------
def test_plugin_interface_call_by_call():
    p = 65
    A, b = _A(p), _b(p, 5)
    rng = np.random.default_rng(12)
    om = rng.random(p) + 0.5
    lam = 0.2 * np.abs(b).max()
    f, fo = cd.CDQuadraticLoss(A, b), O.CDQuadraticLoss(A, b)
    g, go = cd.ProxL1(lam, om), O.ProxL1(lam, om)
    x0 = np.where(rng.random(p) < 0.6, rng.standard_normal(p), 0.0)
    x, xo = cd.SparseIterate(p, x0), O.SparseIterate(p, x0)
    assert cd.numCoordinates(f) == O.numCoordinates(fo) == p

    def grads():
        ref = np.array([O.gradient(fo, xo, k) for k in range(1, p + 1)])
        got = np.array([cd.gradient(f, x, k) for k in range(1, p + 1)])
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())     # 1e-12 relative to the gradient's scale

    cd.initialize_(f, x)
    O.initialize_(fo, xo)
    grads()
    order = rng.permutation(np.r_[np.arange(1, p + 1), np.arange(1, p + 1)])[:40]
    for k in order.tolist():
        h, ho = cd.descendCoordinate_(f, g, x, k), O.descendCoordinate_(fo, go, xo, k)
        assert abs(h - ho) <= 1e-12, (k, h, ho)
        assert x.nzval2ind.tolist() == xo.nzval2ind.tolist()          # zeros keep their slots: no dropzeros! here
    np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL)
    grads()
    sup = xo.nzval2ind.tolist()
    mh, mho = cd.cdPass_(x, f, g, sup), O.cdPass_(xo, fo, go, sup)
    assert abs(mh - mho) <= 1e-12
    assert x.nzval2ind.tolist() == xo.nzval2ind.tolist()              # ... and after a pass it has run
    # a caller's list may name a coordinate twice
    twice = [3, 7, 3, 3, 9, 7] + list(range(1, p + 1)) + [p, p]
    mh, mho = cd.cdPass_(x, f, g, twice), O.cdPass_(xo, fo, go, twice)
    assert abs(mh - mho) <= 1e-12 and x.nzval2ind.tolist() == xo.nzval2ind.tolist()
    np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL)
    grads()
    np.testing.assert_allclose(cd.findLambdaMax(x, f, g), O.findLambdaMax(xo, fo, go), rtol=1e-12)
    np.testing.assert_allclose(cd.objective(f, g), O.objective(fo, go, xo), rtol=1e-12)
    f.close()


# ---- 6. least-squares form == covariance form (test/lasso.jl:36-56) ----------------------------------------------------------
def test_least_squares_form_equals_covariance_form():
    rng = np.random.default_rng(2)
    n, p, s = 500, 50, 10
    X = np.asfortranarray(rng.standard_normal((n, p)))
    Y = X[:, :s] @ rng.standard_normal(s) + 0.1 * rng.standard_normal(n)
    lam = np.full(p, 0.3)
    beta_ls = cd.lasso(X, Y, 1.0, lam, cd.CDOptions(maxIter=5000, optTol=1e-12)).x.dense()
    A = X.T @ X / n
    A = (A + A.T) / 2
    f = cd.CDQuadraticLoss(A, -X.T @ Y / n)
    x = cd.SparseIterate(p)
    cd.coordinateDescent_(x, f, cd.ProxL1(1.0, lam), cd.CDOptions(maxIter=5000, optTol=1e-12))
    np.testing.assert_allclose(x.dense(), beta_ls, rtol=0, atol=1e-5)
    kkt = np.max(np.abs(X.T @ (Y - X @ x.dense()))) / n
    assert abs(kkt - 0.3) / 0.3 <= 1e-5
    f.close()


# ---- 7. limits and co-existence ----------------------------------------------------------------------------------------------
def test_limits_are_named():
    L = cd._lib.lib()
    h = C.c_void_p()
    assert L.cdh_quad_create(C.byref(h), PMAX + 1, 1, 0) == cd._lib.CDH_BAD_ARG and not h.value
    assert str(PMAX).encode() in L.cdh_last_error(None)
    with pytest.raises(cd.ArgumentError, match=str(PMAX)):
        cd.CDQuadraticLoss(np.eye(PMAX + 1), np.zeros(PMAX + 1))
    A = _A(P_B)
    with pytest.raises(cd.ArgumentError, match="max_batch = 3"):
        cd.CDQuadraticLoss(A, np.zeros((P_B, 4)), max_batch=3)
    f = cd.CDQuadraticLoss(A, np.ones((P_B, 3)), max_batch=3)
    with pytest.raises(cd.ArgumentError, match="max_batch = 3"):
        f.set_b(np.ones((P_B, 4)))
    bad = np.ones((P_B, 4), order="F")
    assert L.cdh_quad_set_b(f._h, 4, bad.ctypes.data_as(C.c_void_p), P_B) == cd._lib.CDH_BAD_ARG     # the library's own refusal
    assert b"max_batch = 3" in L.cdh_last_error(None)
    with pytest.raises(cd.DimensionMismatch):
        cd.coordinateDescent_([cd.SparseIterate(P_B), cd.SparseIterate(P_B + 1), cd.SparseIterate(P_B)], f, cd.ProxL1(0.1))
    with pytest.raises(cd.DimensionMismatch):
        cd.coordinateDescent_([cd.SparseIterate(P_B)] * 3, f, cd.ProxL1(0.1, np.ones(P_B + 1)))
    with pytest.raises(cd.ArgumentError):
        cd.coordinateDescent_([cd.SparseIterate(P_B)] * 2, f, cd.ProxL1(0.1))
    f.close()


def test_quad_and_least_squares_handles_side_by_side():
    rng = np.random.default_rng(8)
    n, p = 300, 40
    X = np.asfortranarray(rng.standard_normal((n, p)))
    Y = X[:, :5] @ rng.standard_normal(5) + rng.standard_normal(n)
    A, b = _A(p), _b(p, 77)
    fq, fl = cd.CDQuadraticLoss(A, b), cd.CDLeastSquaresLoss(Y, X)
    oq, ol = O.CDQuadraticLoss(A, b), O.CDLeastSquaresLoss(Y, X)
    xq, xl, xoq, xol = cd.SparseIterate(p), cd.SparseIterate(p), O.SparseIterate(p), O.SparseIterate(p)
    for lam in (0.5, 0.2, 0.08):
        o = dict(OPT, randomize=True, seed=3)
        lq = lam * np.abs(b).max()
        cd.coordinateDescent_(xq, fq, cd.ProxL1(lq), cd.CDOptions(**o))
        cd.coordinateDescent_(xl, fl, cd.ProxL1(lam), cd.CDOptions(**o))
        _same(fq.last_stats, xq, O.coordinateDescent_(xoq, oq, O.ProxL1(lq), O.CDOptions(**o)), xoq)
        _same(fl.last_stats, xl, O.coordinateDescent_(xol, ol, O.ProxL1(lam), O.CDOptions(**o)), xol)
    fq.close()
    fl.close()
