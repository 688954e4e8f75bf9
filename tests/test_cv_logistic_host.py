"""cvLogisticLassoPath without a GPU: the identity that makes a fold of the logistic lasso a 0/1 weight with z = eta on the
held-out rows -- on the CPU oracle's weighted loss alone --, the selection rules on the deviance curves of the numpy twin
(tests/_cv_logistic_numpy.py: fitted on the training rows only), whose minima are asserted here so that the GPU cases
(tests/test_gpu_cv_logistic.py) are known to decide something, every refusal of the front end that precedes the device, and
the new prototype."""
import os
import re

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cv_logistic_numpy as CL
import _cv_numpy as CV
import _logistic_numpy as LG
from coordinatedescent_jl_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")


@pytest.mark.parametrize("name", list(CL.CASES))
def test_masked_route_is_the_fit_on_the_training_rows(name):
    """All n rows with w = 0 and z = eta on the fold, omega = sqrt(sum_train x^2 / n) and lambda sqrt(n_k / n), against the
    logistic lasso on the n_k training rows with their own column rms, at 0.5 and 0.1 of lambda_max, every fold: the same
    rounds and beta within 1e-12.  Measured when this was written: 4.5e-16 at the largest."""
    X, y, icpt, K, ids, _ = CL.data(name)
    lmax = LG.lambda_max(X, y, intercept=icpt)
    worst = 0.0
    for frac in (0.5, 0.1):
        for k in range(K):
            held = ids == k
            Xt, yt = np.asfortranarray(X[~held]), y[~held]
            om = np.sqrt((Xt * Xt).sum(axis=0) / Xt.shape[0])
            b, b0, rounds, conv, _ = LG.logistic_lasso(Xt, yt, frac * lmax, om, optTol=1e-11, intercept=icpt)
            mb, mb0, mrounds = CL.masked_lasso(X, y, held, frac * lmax, optTol=1e-11, intercept=icpt)
            assert conv and rounds == mrounds and np.count_nonzero(b) >= 1, (name, frac, k, rounds, mrounds)
            worst = max(worst, float(np.max(np.abs(b - mb))), abs(b0 - mb0))
    print(f"masked route vs training rows only [{name}]: {worst:.2e}")
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("name", list(CL.CASES))
def test_selection_on_the_twins_deviance_curves(name):
    """The deviance minimum of every case is interior, unique and >= 5e-4 below the runner-up, so a 1e-10 error in a
    coefficient cannot move it; api._cv_select and the twin's rules agree on the twin's curves, for both measures."""
    X, y, icpt, K, ids, lams = CL.data(name)
    t = CL.cv(name)
    cvm, cvsd, imin, i1se = t["deviance"]
    assert imin == CL.INDEX_MIN[name] and 0 < imin < len(lams) - 1, (name, imin, cvm)
    others = np.delete(cvm, imin)
    print(f"twin deviance curve [{name}]: index_min {imin} index_1se {i1se}, runner-up {others.min() - cvm[imin]:.2e} away; "
          f"class: index_min {t['class'][2]} index_1se {t['class'][3]}; smallest held-out |eta| {t['min_abs_eta'].min():.2e}")
    assert others.min() - cvm[imin] >= 5e-4
    assert i1se <= imin
    for measure, err in (("deviance", t["fold_deviance"]), ("class", t["fold_class"])):
        a_cvm, a_cvsd, a_imin, a_i1se = api._cv_select(lams, t["sizes"], err)
        np.testing.assert_allclose(a_cvm, t[measure][0], rtol=1e-14)
        np.testing.assert_allclose(a_cvsd, t[measure][1], rtol=1e-12, atol=1e-300)
        assert (a_imin, a_i1se) == t[measure][2:], measure
    # the class error is a count over the fold, the deviance of the training rows falls along the path
    counts = t["fold_class"] * t["sizes"][:, None]
    assert np.all(np.abs(counts - np.round(counts)) <= 1e-9)
    assert np.all(np.diff(t["train_deviance"], axis=1) < 0)
    assert np.array_equal(ids, CV.fold_ids(len(y), K, 0))


def test_miss_counts_eta_zero_as_class_zero():
    y = np.array([1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.25])
    eta = np.array([0.0, 0.0, 2.0, 2.0, -2.0, -2.0, 1.0])
    np.testing.assert_array_equal(CL.miss(y, eta), [1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.75])


def test_refusals_that_precede_the_device():
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((12, 3)), (np.arange(12) % 2).astype(float)
    lam = [0.5, 0.1]
    ok = np.arange(12) % 3
    for measure in ("auc", "mse", "", None, "Deviance"):
        with pytest.raises(cd.ArgumentError, match="measure"):
            cd.cvLogisticLassoPath(X, y, lam, K=3, measure=measure)
    for kw in (dict(K=1), dict(K=0), dict(K=256), dict(K=13),                                                # K < 2, K > 255, K > n
               dict(K=4, folds=ok), dict(K=3, folds=np.where(ok == 1, 0, ok)),                               # an empty fold
               dict(K=3, folds=ok[:11]), dict(K=3, folds=np.where(ok == 2, 3, ok)), dict(K=3, folds=ok + 0.5)):
        with pytest.raises(cd.ArgumentError):
            cd.cvLogisticLassoPath(X, y, lam, **kw)
    with pytest.raises(cd.ArgumentError, match="fold 3 is empty"):
        cd.cvLogisticLassoPath(X, y, lam, K=4, folds=ok)
    with pytest.raises(cd.ArgumentError, match="lambdapath is empty"):
        cd.cvLogisticLassoPath(X, y, [], K=3)
    # any loss but CDLogisticLoss is a TypeError, before its handle is looked at (objects made without a device)
    for cls in (cd.CDLeastSquaresLoss, cd.CDSqrtLassoLoss, cd.CDWeightedLSLoss, cd.CDVaryingCoefficientLoss, cd.CDQuadraticLoss):
        with pytest.raises(TypeError):
            cd.cvLogisticLassoPath(cls.__new__(cls), None, lam, K=3)
    # an intercept's start from a fold whose training labels are all of one kind: refused before the upload
    y1 = (ok == 0).astype(float)                         # the ones are exactly fold 0
    with pytest.raises(cd.ArgumentError, match="labels of both kinds"):
        cd.cvLogisticLassoPath(X, y1, lam, K=3, folds=ok, fit_intercept=True)
    f = cd.CDLogisticLoss.__new__(cd.CDLogisticLoss)
    f.n = 12
    with pytest.raises(cd.ArgumentError, match="column of ones"):
        cd.cvLogisticLassoPath(f, None, lam, K=3, fit_intercept=True)


def test_record_constant_sits_beside_the_plain_one():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "glm_plan.hpp")).read())
    assert re.search(r"constexpr int kGlmVals = 3;", code) and re.search(r"constexpr int kGlmFoldVals = 5;", code)


def test_new_symbol_is_declared_bound_and_cited():
    names = cd.declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    L = cd._lib.lib()
    name = "cdh_glm_irls_fold"
    assert name in names and len(getattr(L, name).argtypes) == 5
    before = hdr[: hdr.index("int32_t %s(" % name)]
    comment = before[before.rindex("/*"):]
    assert "no reference counterpart" in comment
    assert "cd_differentiable_function.jl:118-194" in comment and "lasso.jl:229-260" in comment
    assert re.search(r"^int32_t %s\([^{;]*\) \{ return guarded\(h, \[&\]\(\) -> int32_t \{$" % name, src, flags=re.M)
    jl = open(os.path.join(ROOT, "julia", "CoordinateDescentHIP.jl")).read()
    assert "(:%s, libcdhip)" % name in jl
    for n in ("cvLogisticLassoPath", "CVLogisticLassoPathResult"):
        assert hasattr(cd, n), n
    assert "held_nll" in cd.LogisticLassoSolution.__dataclass_fields__ and "held_miss" in cd.LogisticLassoSolution.__dataclass_fields__
