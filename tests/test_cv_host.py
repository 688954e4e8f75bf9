"""cvLassoPath without a GPU: the selection rules of its numpy twin (tests/_cv_numpy.py) and of api.py on hand-made errors,
the rescaling rule that makes a 0/1-weighted handle a fold -- on the CPU oracle alone --, every refusal of the front end that
precedes the device, the host arithmetic of the kernel (csrc/cv_plan.hpp) as a stand-alone program under the host sanitizers,
and the three new prototypes."""
import os
import re
import subprocess

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
import _cv_numpy as CV
from coordinatedescent_jl_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")


def _both(lam, sizes, mse):
    """The twin's answer, after checking that api.py's own arithmetic gives the same."""
    lam, sizes, mse = np.asarray(lam, float), np.asarray(sizes), np.asarray(mse, float)
    cvm, cvsd = CV.cv_curve(sizes, mse)
    imin, i1se = CV.select(lam, cvm, cvsd)
    a_cvm, a_cvsd, a_imin, a_i1se = api._cv_select(lam, sizes, mse)
    np.testing.assert_allclose(a_cvm, cvm, rtol=1e-14)
    np.testing.assert_allclose(a_cvsd, cvsd, rtol=1e-13, atol=1e-300)
    assert (a_imin, a_i1se) == (imin, i1se)
    return cvm, cvsd, imin, i1se


def test_selection_rules_on_hand_made_errors():
    lam = [8.0, 4.0, 2.0, 1.0, 0.5]
    # equal folds: cvm is the plain mean, cvsd the sample standard deviation over sqrt(K) ... of K = 2: |a - b| / 2
    cvm, cvsd, imin, i1se = _both(lam, [5, 5], [[4.0, 2.0, 1.0, 3.0, 5.0], [6.0, 4.0, 2.0, 3.0, 5.0]])
    np.testing.assert_allclose(cvm, [5.0, 3.0, 1.5, 3.0, 5.0])
    np.testing.assert_allclose(cvsd, [1.0, 1.0, 0.5, 0.0, 0.0])
    assert (imin, i1se) == (2, 2)                        # threshold 2.0: nothing but the minimum is within it
    # a tie at the minimum: the first; and the 1-se lambda is the largest lambda within the threshold
    cvm, cvsd, imin, i1se = _both(lam, [5, 5], [[4.0, 1.0, 1.0, 1.0, 5.0], [6.0, 3.0, 3.0, 3.0, 5.0]])
    assert (imin, i1se) == (1, 1) and cvm[1] == cvm[2] == cvm[3]
    cvm, cvsd, imin, i1se = _both(lam, [5, 5], [[2.75, 2.5, 1.0, 2.0, 5.0], [3.25, 3.5, 3.0, 2.0, 5.0]])
    assert imin == 2 and cvsd[2] == 1.0 and i1se == 0    # 3.0 <= 2.0 + 1.0: equality counts
    # a lambda path that is not decreasing: "largest lambda", not "lowest index"; equal lambdas: the lowest index
    _, _, imin, i1se = _both([1.0, 8.0, 2.0, 8.0], [5, 5], [[0.5, 1.5, 1.0, 1.5], [1.5, 1.5, 1.0, 1.5]])
    assert (imin, i1se) == (0, 1)
    # unequal folds weigh by size
    cvm, cvsd, imin, i1se = _both([2.0, 1.0], [1, 3], [[4.0, 0.0], [0.0, 4.0]])
    np.testing.assert_allclose(cvm, [1.0, 3.0])
    np.testing.assert_allclose(cvsd, np.sqrt([0.25 * 9 + 0.75 * 1, 0.25 * 9 + 0.75 * 1]))
    assert (imin, i1se) == (0, 0)
    # three folds: the divisor is K - 1
    cvm, cvsd, _, _ = _both([1.0], [2, 2, 2], [[1.0], [2.0], [3.0]])
    np.testing.assert_allclose(cvsd, [np.sqrt((1 + 0 + 1) / 3 / 2)])


def test_fold_ids_of_a_seed():
    for n, K, seed in ((601, 3, 4), (10, 10, 0), (257, 255, 9)):
        ids = CV.fold_ids(n, K, seed)
        got, sizes = api._cv_fold_ids(n, K, None, seed)
        np.testing.assert_array_equal(got, ids)
        np.testing.assert_array_equal(sizes, np.bincount(ids, minlength=K))
        assert sizes.max() - sizes.min() <= 1 and got.dtype == np.int32


PROBLEMS = ((601, 40, 3), (200, 30, 4), (1000, 20, 10))


@pytest.mark.parametrize("n,p,K", PROBLEMS)
@pytest.mark.parametrize("standardize", (True, False))
def test_rescaling_rule_on_the_oracle(n, p, K, standardize):
    """LassoPath on the training rows == the weighted loss on all rows with 0/1 weights, omega = _stdX!(w, X) (or 1) and the
    rescaled lambda.  Measured when this was written: 8e-15 at the largest."""
    rng = np.random.default_rng(n)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    bstar = np.zeros(p)
    bstar[:5] = (2.0, -1.5, 1.0, 0.5, -0.25)
    Y = X @ bstar + rng.standard_normal(n)
    folds = rng.permutation(n) % K
    lmax = np.max(np.abs(X.T @ Y)) / n
    lams = lmax * np.geomspace(0.9, 0.005, 12)
    opts = O.CDOptions(maxIter=5000, optTol=1e-12, randomize=False)
    worst = 0.0
    for k in (0, K - 1):
        tr = folds != k
        _, want = O.LassoPath(np.asfortranarray(X[tr]), Y[tr], lams, opts, standardizeX=standardize)
        w = tr.astype(np.float64)
        om = CV.wstd(w, X) if standardize else np.ones(p)
        f, x = O.CDWeightedLSLoss(Y, X, w), O.SparseIterate(p)
        for lam, b in zip(CV.rescale(lams, tr.sum(), n, standardize), want):
            O.coordinateDescent_(x, f, O.ProxL1(lam, om), opts)
            worst = max(worst, float(np.max(np.abs(x.dense() - b))))
        assert np.count_nonzero(want[-1]) >= 5
    assert worst <= 1e-12, worst


def test_refusals_that_precede_the_device():
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((12, 3)), rng.standard_normal(12)
    lam = [0.5, 0.1]
    ok = np.arange(12) % 3
    bad = (dict(K=3, folds=ok[:11]), dict(K=3, folds=np.r_[ok, 0]), dict(K=3, folds=ok.reshape(3, 4)),      # wrong length / shape
           dict(K=3, folds=np.where(ok == 2, 3, ok)), dict(K=3, folds=np.where(ok == 0, -1, ok)),            # ids outside 0 .. K - 1
           dict(K=4, folds=ok), dict(K=3, folds=np.where(ok == 1, 0, ok)),                                   # an empty fold
           dict(K=1), dict(K=0), dict(K=256), dict(K=13),                                                    # K < 2, K > 255, K > n
           dict(K=3, folds=ok + 0.5))
    for kw in bad:
        with pytest.raises(cd.ArgumentError):
            cd.cvLassoPath(X, Y, lam, **kw)
    with pytest.raises(cd.ArgumentError, match="fold 3 is empty"):
        cd.cvLassoPath(X, Y, lam, K=4, folds=ok)
    with pytest.raises(cd.ArgumentError, match="lambdapath is empty"):
        cd.cvLassoPath(X, Y, [], K=3)
    # any loss but CDLeastSquaresLoss is a TypeError, before its handle is looked at (objects made without a device)
    for cls in (cd.CDSqrtLassoLoss, cd.CDWeightedLSLoss, cd.CDVaryingCoefficientLoss, cd.CDQuadraticLoss):
        with pytest.raises(TypeError):
            cd.cvLassoPath(cls.__new__(cls), None, lam, K=3)


def test_sanitized_stand_alone_program(tmp_path):
    exe = str(tmp_path / "cv_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cv_plan_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "cv_plan_main OK" in out


def test_plan_header_holds_no_hip():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "cv_plan.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|hip[A-Z_]|threadIdx|blockIdx", code)


def test_new_symbols_are_declared_bound_and_cited():
    names = cd.declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    L = cd._lib.lib()
    for name, nargs in (("cdh_set_folds", 4), ("cdh_set_fold_weights", 2), ("cdh_path_sse", 9)):
        assert name in names and len(getattr(L, name).argtypes) == nargs, name
        before = hdr[: hdr.index("int32_t %s(" % name)]
        comment = before[before.rindex("/*"):]
        assert "lasso.jl:229-260" in comment and "utils.jl:140-151" in comment, name
    for n in ("cvLassoPath", "CVLassoPathResult"):
        assert hasattr(cd, n), n
    assert hasattr(cd.CDLeastSquaresLoss, "path_sse") and hasattr(cd.CDLeastSquaresLoss, "set_fold_weights")
