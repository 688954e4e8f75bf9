"""CPU-side checks of the leave-one-out bandwidth selection: the yardstick of the GPU tests (tests/_vc_cv_numpy.py) against
closed forms on tiny inputs, the structural facts of the reference's loop (src/varying_coefficient_lasso.jl:82-137) that
the device code relies on, and the new symbols."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
from _vc_numpy import expand, gen_data, weights
from _vc_cv_numpy import find_init_residuals, get_sigma, oracle_lvocv, screening_scores, screening_set


def test_get_sigma_with_unit_weights_is_the_sigma_of_scaled_lasso():
    """utils.jl:167-175 against lasso.jl:134: sqrt(sum(abs2, r) / n)."""
    r = np.array([3.0, -4.0, 12.0, 0.0])
    assert get_sigma(np.ones(4), r) == np.sqrt(169.0 / 4.0)
    assert get_sigma(np.array([1.0, 0.0, 2.0, 5.0]), r) == np.sqrt((9.0 + 288.0) / 8.0)


def test_a_left_out_row_changes_nothing_but_its_own_term():
    w = np.array([0.5, 2.0, 1.0, 4.0])
    r = np.array([1.0, -2.0, 3.0, 0.5])
    X = np.array([[1.0, 2.0], [3.0, -1.0], [0.0, 4.0], [2.0, 2.0]])
    y = np.array([1.0, 2.0, -1.0, 3.0])
    for i in range(4):
        wl = w.copy()
        wl[i] = 0.0
        # _getSigma: both sums lose exactly row i's term
        assert get_sigma(wl, r) == np.sqrt(((w * r * r).sum() - w[i] * r[i] ** 2) / (w.sum() - w[i]))
        # the scores: sum_i X_ij w_i y_i loses X_ij w_i y_i
        full = (X * (w * y)[:, None]).sum(axis=0)
        assert np.array_equal(screening_scores(wl, X, y), np.abs(full - X[i] * w[i] * y[i]))


def test_weighted_screening_on_an_orthogonal_design():
    """X = the first four columns of I_6: the scores are |w_j y_j|, the fit on the screened columns reproduces y on their
    rows, and the residual is y elsewhere.  s = 2 with a tie for second place keeps three columns (`.>=`, utils.jl:123)."""
    X = np.eye(6)[:, :4]
    w = np.array([1.0, 2.0, 4.0, 0.5, 1.0, 1.0])
    y = np.array([8.0, -2.0, 1.0, 3.0, 5.0, -7.0])
    scores = screening_scores(w, X, y)
    assert np.array_equal(scores, [8.0, 4.0, 4.0, 1.5])
    assert screening_set(scores, 2).tolist() == [True, True, True, False]
    assert screening_set(scores, 1).tolist() == [True, False, False, False]
    r, S, _ = find_init_residuals(w, X, y, 2)
    assert S.tolist() == [True, True, True, False]
    assert np.allclose(r, [0.0, 0.0, 0.0, 3.0, 5.0, -7.0], rtol=0, atol=1e-14)
    assert get_sigma(w, np.array([0.0, 0.0, 0.0, 3.0, 5.0, -7.0])) == np.sqrt((4.5 + 25.0 + 49.0) / 9.5)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_expanded_row_at_its_own_z_is_the_base_row_interleaved_with_zeros(dtype):
    """z[i] - z0 is exactly 0 at z0 = z[i], so v *= 0 gives exact zeros at every power above 0: the prediction
    dot(wX[i, S], .) (:132) reads the base row only."""
    X, z, _ = gen_data(np.random.default_rng(0), 40, 2, 3, dtype)
    for degree in range(4):
        for i in (0, 17, 39):
            row = expand(X, z, z[i], degree)[i].reshape(X.shape[1], degree + 1)
            assert np.array_equal(row[:, 0], X[i]) and not row[:, 1:].any()


def test_an_empty_support_predicts_zero():
    """The case the reference never handles: with lambda0 so large that every solve ends at beta = 0, Yh = 0 for every
    point and MSE[h] = sum(y.^2)."""
    X, z, y = gen_data(np.random.default_rng(1), 30, 2, 1)
    MSE, pts = oracle_lvocv(O, X, z, y, 1, "gaussian", [0.1, 0.4], 1e3, maxIter=200, optTol=1e-10, randomize=False)
    assert all(not p["S"].any() and p["yhat"] == 0.0 and p["refit"] is None for p in pts)
    assert np.allclose(MSE, float(y @ y), rtol=1e-14, atol=0)
    assert "empty support" in cd.lvocv_locpolyl1.__doc__ and "Yh = 0" in cd.lvocv_locpolyl1.__doc__


def test_the_yardstick_leaves_the_row_out():
    X, z, y = gen_data(np.random.default_rng(2), 25, 2, 0)
    _, pts = oracle_lvocv(O, X, z, y, 0, "epanechnikov", [0.5], 0.1, maxIter=500, optTol=1e-10, randomize=False)
    assert [p["row"] for p in pts] == list(range(25)) and all(1 <= p["sigma_iters"] <= 10 for p in pts)
    assert all(len(p["sigmas"]) == p["sigma_iters"] + 1 == len(p["margins"]) + 1 for p in pts)
    w = weights("epanechnikov", 0.5, z, z[3])
    assert w[3] == 1.5                                     # the peak 0.75 / h, which the loop zeroes


def test_new_symbols_are_declared_and_exported():
    names = cd.declared_symbols()
    L = C.CDLL(cd.SO_PATH)
    for n in ("cdh_vc_set_point_loo", "cdh_resid_wmoments", "cdh_get_X_row"):
        assert n in names and hasattr(L, n), n
    for n in ("lvocv_locpolyl1", "getSigma", "findInitResiduals_"):
        assert hasattr(cd, n), n
    assert hasattr(cd.CDVaryingCoefficientLoss, "set_point_leave_out")


def test_lvocv_locpolyl1_checks_its_arguments_before_touching_the_device():
    X, y = np.zeros((10, 3)), np.zeros(10)
    with pytest.raises(cd.DimensionMismatch):
        cd.lvocv_locpolyl1(X, np.zeros(9), y, 1, [0.1], cd.GaussianKernel, 0.1)
    with pytest.raises(cd.DimensionMismatch):
        cd.lvocv_locpolyl1(X, np.zeros(10), np.zeros(11), 1, [0.1], cd.GaussianKernel, 0.1)
    with pytest.raises(cd.ArgumentError):
        cd.lvocv_locpolyl1(X, np.zeros(10), y, 4, [0.1], cd.GaussianKernel, 0.1)
