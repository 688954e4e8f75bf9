"""The Cox lasso without a GPU: the three new prototypes -- declared, bound with the right arity, cited, guarded, in the Julia
binding and in INTEGRATION.md -- the names of the front end, and its refusals that precede the device."""
import os
import re

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")

NEW_SYMBOLS = (("cdh_glm_set_survival", 4), ("cdh_glm_get_survival", 3), ("cdh_glm_cox_irls", 6))


def test_new_symbols_are_declared_bound_and_cited():
    names = cd.declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    L = cd._lib.lib()
    for name, nargs in NEW_SYMBOLS:
        assert name in names and len(getattr(L, name).argtypes) == nargs, name
        before = hdr[: hdr.index("int32_t %s(" % name)]
        comment = before[before.rindex("/*"):]
        assert "no reference counterpart" in comment and "cd_differentiable_function.jl:118-194" in comment, name
        assert re.search(r"^int32_t %s\([^{;]*\) \{ return guarded\(h, \[&\]\(\) -> int32_t \{$" % name, src, flags=re.M), name
    jl = open(os.path.join(ROOT, "julia", "CoordinateDescentHIP.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in NEW_SYMBOLS:
        assert "(:%s, libcdhip)" % name in jl, name
        assert "`%s`" % name in doc, name


def test_the_sources_keep_the_step_in_files_of_its_own():
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    assert src.index('#include "glm_kernels.hpp"') < src.index('#include "cox_kernels.hpp"') < src.index('#include "solve.hpp"')
    assert src.index('#include "glm_plan.hpp"') < src.index('#include "cox_plan.hpp"') < src.index("struct GlmState {")
    assert "Cox = 2" in src and src.count('"CDH_COX_GRID"') == 1
    k = open(os.path.join(CSRC, "cox_kernels.hpp")).read()
    assert "cox_plan(h->ld, h->knobs.cox_grid)" in k and "getenv" not in k
    assert '"partials too small"' in k
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("Strata", "start–stop", "Efron", "observation weights"):
        assert word in design[design.index("## 9"):], word


def test_api_names():
    for n in ("CDCoxLoss", "coxLasso_", "coxLasso", "coxLambdaMax", "CoxLassoPath", "cvCoxLassoPath", "CoxLassoSolution",
              "CoxLassoPathResult", "CVCoxLassoPathResult"):
        assert hasattr(cd, n), n
    assert issubclass(cd.CDCoxLoss, cd.CDWeightedLSLoss)
    assert not issubclass(cd.CDCoxLoss, cd.CDLogisticLoss) and not issubclass(cd.CDCoxLoss, cd.CDPoissonLoss)
    for prop in ("time", "status", "offset"):
        assert isinstance(getattr(cd.CDCoxLoss, prop), property), prop
    assert hasattr(cd.CDCoxLoss, "irls_step") and hasattr(cd.CDCoxLoss, "objective")
    import inspect
    sig = inspect.signature(cd.CDCoxLoss.irls_step).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("apply", True), ("wmin", 1e-5), ("eta_max", 50.0), ("fold", None)]
    for fn in (cd.coxLasso, cd.CoxLassoPath, cd.cvCoxLassoPath, cd.coxLambdaMax):
        assert "fit_intercept" not in inspect.signature(fn).parameters
    for fld in ("nll", "rounds", "converged", "monotone", "capped", "events", "held_deviance"):
        assert fld in cd.CoxLassoSolution.__dataclass_fields__, fld
    assert set(cd.CVPoissonLassoPathResult.__dataclass_fields__) | {"fold_events"} == set(cd.CVCoxLassoPathResult.__dataclass_fields__)
    assert issubclass(cd.CoxLassoPathResult, cd.LassoPathResult)
    o = cd.IRLSOptions()                                        # the defaults the other families pin stay as they are
    assert (o.maxIter, o.optTol, o.wmin, o.etaMax) == (25, 1e-7, 1e-5, 50.0)


def test_refusals_that_precede_the_device():
    rng = np.random.default_rng(0)
    n = 12
    X = rng.standard_normal((n, 3))
    y = np.c_[rng.exponential(1.0, n), (rng.random(n) < 0.7).astype(float)]
    y[0, 1] = 1.0
    calls = (lambda yy, XX: cd.CDCoxLoss(yy, XX), lambda yy, XX: cd.coxLasso(XX, yy, 0.1),
             lambda yy, XX: cd.CoxLassoPath(XX, yy, [0.1]), lambda yy, XX: cd.cvCoxLassoPath(XX, yy, [0.1], K=3))
    for call in calls:
        with pytest.raises(cd.DimensionMismatch):
            call(np.c_[y, np.ones(n)], X)                       # n x 3
        with pytest.raises(cd.DimensionMismatch):
            call(y[:, 0], X)                                    # a vector
        with pytest.raises(cd.DimensionMismatch):
            call(y[:11], X)
        bad = y.copy()
        bad[4, 1] = 0.5
        with pytest.raises(cd.ArgumentError, match=r"status\[4\]"):
            call(bad, X)
        bad = y.copy()
        bad[3, 0] = np.nan
        with pytest.raises(cd.ArgumentError, match=r"time\[3\]"):
            call(bad, X)
        none = y.copy()
        none[:, 1] = 0.0
        with pytest.raises(cd.ArgumentError, match="no row is an event"):
            call(none, X)
    with pytest.raises(TypeError):
        cd.CDCoxLoss(y, X.astype(np.float32))
    with pytest.raises(cd.DimensionMismatch):
        cd.CDCoxLoss(y, X, offset=np.zeros(n - 1))
    with pytest.raises(cd.ArgumentError, match="offset"):
        cd.CDCoxLoss(y, X, offset=np.r_[np.zeros(n - 1), np.inf])
    # a fold without a held-out event, or holding all of them, before the upload
    yk = y.copy()
    yk[:, 1] = 0.0
    yk[[0, 3], 1] = 1.0                                         # both events in fold 0 of arange % 3
    with pytest.raises(cd.ArgumentError, match="fold 0 holds every event|fold 1 holds no event"):
        cd.cvCoxLassoPath(X, yk, [0.1], K=3, folds=np.arange(n) % 3)
    yk[1, 1] = 1.0                                              # folds 0 and 1 have events, fold 2 none
    with pytest.raises(cd.ArgumentError, match="fold 2 holds no event"):
        cd.cvCoxLassoPath(X, yk, [0.1], K=3, folds=np.arange(n) % 3)
    with pytest.raises(cd.ArgumentError, match="measure"):
        yk[2, 1] = 1.0
        cd.cvCoxLassoPath(X, yk, [0.1], K=3, folds=np.arange(n) % 3, measure="class")
    # siblings refuse each other, on objects made without a device
    for cls in (cd.CDLeastSquaresLoss, cd.CDWeightedLSLoss, cd.CDLogisticLoss, cd.CDPoissonLoss):
        f = cls.__new__(cls)
        with pytest.raises(TypeError):
            cd.coxLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1))
        with pytest.raises(TypeError):
            cd.coxLambdaMax(f)
        with pytest.raises(TypeError):
            cd.coxLasso(f, None, 0.1)
        with pytest.raises(TypeError):
            cd.cvCoxLassoPath(f, None, [0.1], K=3)
    f = cd.CDCoxLoss.__new__(cd.CDCoxLoss)
    with pytest.raises(TypeError):
        cd.poissonLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1))
    with pytest.raises(TypeError):
        cd.logisticLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1))
    with pytest.raises(cd.ArgumentError, match="warmStart"):
        cd.coxLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1), cd.CDOptions(warmStart=False))
    with pytest.raises(cd.ArgumentError, match="belongs to the loss"):
        cd.coxLasso(f, None, 0.1, offset=np.zeros(12))
