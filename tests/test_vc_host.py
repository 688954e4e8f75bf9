"""CPU-side checks of the varying-coefficient lasso: the smoothing kernels and get_nonzero_coordinates on the host, the
numpy yardstick of the GPU tests (tests/_vc_numpy.py) against the reference's own Kronecker check, and the new symbols."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
from _vc_numpy import expand, weights, wstd


def test_gaussian_kernel_value_of_the_reference_test():
    """test/varying_coefficient_lasso.jl:16-20."""
    assert cd.evaluate(cd.GaussianKernel(1.), .3, .4) == np.exp(-0.01)
    k = cd.createKernel(cd.GaussianKernel, 0.5)
    assert isinstance(k, cd.GaussianKernel) and k.h == 0.5
    x = np.linspace(0, 1, 11)
    assert np.array_equal(cd.evaluate(k, x, 0.25), np.exp(-(x - 0.25) ** 2 / 0.5) / 0.5)   # h, not 2 h^2; scaled by 1 / h


def test_epanechnikov_kernel_is_zero_from_u_equal_one():
    k = cd.createKernel(cd.EpanechnikovKernel, 0.25)
    assert cd.evaluate(k, 0.5, 0.25) == 0.0 and cd.evaluate(k, 0.0, 0.25) == 0.0      # |u| == 1 exactly
    assert cd.evaluate(k, 0.25, 0.25) == 0.75 / 0.25
    assert cd.evaluate(k, 0.375, 0.25) == 0.75 * (1 - 0.25) / 0.25
    assert np.array_equal(cd.evaluate(k, np.array([0.0, 0.25, 0.6]), 0.25), [0.0, 3.0, 0.0])
    with pytest.raises(TypeError):
        cd.createKernel(cd.SmoothingKernel, 1.0)


def test_numpy_yardstick_agrees_with_the_host_kernels():
    z = np.random.default_rng(0).random(100)
    assert np.array_equal(weights("gaussian", 0.1, z, 0.3), cd.evaluate(cd.GaussianKernel(0.1), z, 0.3))
    assert np.array_equal(weights("epanechnikov", 0.25, z, 0.3), cd.evaluate(cd.EpanechnikovKernel(0.25), z, 0.3))


def test_get_nonzero_coordinates_both_modes():
    """src/varying_coefficient_lasso.jl:479-512: a group counts as soon as any of its degree + 1 coefficients is non-zero."""
    x = cd.SparseIterate(8)           # p = 4 groups of degree + 1 = 2
    x[2] = 1.5                        # group 1 (second coefficient)
    x[7] = -2.0                       # group 4 (first coefficient)
    x[5] = 1.0
    x[5] = 0.0                        # a stored zero does not count
    assert cd.get_nonzero_coordinates(x, 4, 1, True).tolist() == [True, True, False, False, False, False, True, True]
    assert cd.get_nonzero_coordinates(x, 4, 1, False).tolist() == [True, False, False, True]
    assert cd.get_nonzero_coordinates(np.zeros(6), 2, 2, True).tolist() == [False] * 6
    assert cd.get_nonzero_coordinates(x.dense(), 8, 0, False).tolist() == [False, True, False, False, False, False, True, False]
    with pytest.raises(cd.DimensionMismatch):
        cd.get_nonzero_coordinates(x, 3, 1, True)


def test_numpy_expansion_reproduces_the_reference_kronecker_check():
    """test/varying_coefficient_lasso.jl:43-66: X = reshape(1:6, 2, 3), z = [0.2, 0.4], z0 = 0.3."""
    X = np.arange(1., 7.).reshape(3, 2).T.copy(order="F")
    z, z0 = np.array([0.2, 0.4]), 0.3
    assert np.array_equal(expand(X, z, z0, 0), X)
    for degree, Q in ((1, [[1., -0.1], [1., 0.1]]), (2, [[1., -0.1, 0.01], [1., 0.1, 0.01]])):
        want = np.vstack([np.kron(X[i], Q[i]) for i in range(2)])
        got = expand(X, z, z0, degree)
        assert got.shape == (2, 3 * (degree + 1))
        assert np.allclose(got, want, rtol=1e-14, atol=0)        # the reference's own check is `≈`
    # the recurrence runs in the storage type, and base column j is expanded column j (degree + 1)
    X32 = X.astype(np.float32)
    e32 = expand(X32, z.astype(np.float32), z0, 2)
    assert e32.dtype == np.float32 and np.array_equal(e32[:, ::3], X32)
    df = z.astype(np.float32) - np.float32(z0)
    assert np.array_equal(e32[:, 2], (X32[:, 0] * df) * df)
    w = np.array([2.0, 0.5])
    assert np.allclose(wstd(w, X), np.sqrt((w[:, None] * X * X).sum(axis=0) / 2), rtol=1e-15)


def test_new_symbols_are_declared_and_exported():
    names = cd.declared_symbols()
    L = C.CDLL(cd.SO_PATH)
    for n in ("cdh_vc_set_data", "cdh_vc_set_point", "cdh_col_wrms", "cdh_gram_weighted"):
        assert n in names and hasattr(L, n), n
    for n in ("GaussianKernel", "EpanechnikovKernel", "createKernel", "evaluate", "get_nonzero_coordinates",
              "CDVaryingCoefficientLoss", "locpolyl1"):
        assert hasattr(cd, n), n
    assert issubclass(cd.CDVaryingCoefficientLoss, cd.CDWeightedLSLoss)


def test_locpolyl1_checks_dimensions_before_touching_the_device():
    X, y = np.zeros((10, 3)), np.zeros(10)
    with pytest.raises(cd.DimensionMismatch):
        cd.locpolyl1(X, np.zeros(9), y, [0.5], 1, cd.GaussianKernel(0.1), 0.1, False)
    with pytest.raises(cd.DimensionMismatch):
        cd.CDVaryingCoefficientLoss(y, X, np.zeros(11), 1)
    with pytest.raises(cd.ArgumentError):
        cd.CDVaryingCoefficientLoss(y, X, np.zeros(10), 4)
