"""What the Python layer refuses of start-stop survival data on the host, before any device call: the loss is never made, so
these run without a GPU (the library is not even loaded: _survival3 runs first in CDCoxLoss.__init__ and in the front ends)."""
import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
from coordinatedescent_jl_amd.api import _survival, _survival3


def _good(n=6):
    stop = np.arange(1.0, n + 1.0)
    start = stop - 0.5
    status = (np.arange(n) % 2 == 0).astype(np.float64)
    return np.asfortranarray(np.random.default_rng(0).standard_normal((n, 2))), start, stop, status


FRONTS = (lambda X, y: cd.CDCoxLoss(y, X), lambda X, y: cd.coxLasso(X, y, 0.1), lambda X, y: cd.CoxLassoPath(X, y, [0.2, 0.1]),
          lambda X, y: cd.cvCoxLassoPath(X, y, [0.2, 0.1], K=2))


def test_three_columns_parse_as_start_stop_status():
    X, start, stop, status = _good()
    a, b, c = _survival3(np.c_[start, stop, status], 6)
    np.testing.assert_array_equal(a, start)
    np.testing.assert_array_equal(b, stop)
    np.testing.assert_array_equal(c, status)
    assert all(v.flags.c_contiguous and v.dtype == np.float64 for v in (a, b, c))
    a, b, c = _survival3(np.c_[stop, status], 6)
    assert a is None
    np.testing.assert_array_equal(b, stop)
    t, s = _survival(np.c_[start, stop, status])                # the two-value form keeps its shape: time is the stop time
    np.testing.assert_array_equal(t, stop)
    np.testing.assert_array_equal(s, status)


@pytest.mark.parametrize("front", FRONTS)
def test_a_wrong_column_count_is_refused(front):
    X, start, stop, status = _good()
    for y in (np.c_[start, stop, status, status], stop[:, None], stop):
        with pytest.raises(cd.DimensionMismatch, match="n x 2.*n x 3"):
            front(X, y)
    with pytest.raises(cd.DimensionMismatch, match="size"):
        front(X, np.c_[start, stop, status][:5])


@pytest.mark.parametrize("front", FRONTS)
def test_start_not_below_stop_is_refused_with_the_row_named(front):
    X, start, stop, status = _good()
    for i, value in ((3, stop[3]), (0, stop[0] + 1.0)):
        bad = start.copy()
        bad[i] = value
        with pytest.raises(cd.DimensionMismatch, match=r"start\[%d\] = .* is not below stop\[%d\]" % (i, i)):
            front(X, np.c_[bad, stop, status])


@pytest.mark.parametrize("front", FRONTS)
def test_a_start_that_is_not_finite_is_refused_with_the_row_named(front):
    X, start, stop, status = _good()
    for i, value in ((2, np.nan), (5, -np.inf), (0, np.inf)):
        bad = start.copy()
        bad[i] = value
        with pytest.raises(cd.ArgumentError, match=r"start\[%d\] is not finite" % i):
            front(X, np.c_[bad, stop, status])


def test_the_earlier_refusals_stand_with_three_columns():
    X, start, stop, status = _good()
    bad = stop.copy()
    bad[1] = np.nan
    with pytest.raises(cd.ArgumentError, match=r"time\[1\] is not finite"):
        cd.CDCoxLoss(np.c_[start, bad, status], X)
    with pytest.raises(cd.ArgumentError, match=r"status\[0\]"):
        cd.CDCoxLoss(np.c_[start, stop, status + 0.5], X)
    with pytest.raises(cd.ArgumentError, match="no row is an event"):
        cd.CDCoxLoss(np.c_[start, stop, 0.0 * status], X)
