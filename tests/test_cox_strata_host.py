"""Strata and observation weights of the Cox lasso without a GPU: the two new prototypes -- declared, bound with the right
arity, cited, guarded, in the Julia binding and in INTEGRATION.md -- the new keywords of the front end, and its refusals that
precede the device."""
import inspect
import os
import re

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")

NEW_SYMBOLS = (("cdh_glm_set_survival_strata", 6), ("cdh_glm_get_survival_strata", 3))


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
    # the signatures the earlier tests pin stay, and the record's last slot is documented as the sum of dv
    assert len(L.cdh_glm_set_survival.argtypes) == 4 and len(L.cdh_glm_cox_irls.argtypes) == 6
    assert "sum of dv_i" in hdr[hdr.index("/* cdh_glm_cox_irls"):hdr.index("int32_t cdh_glm_cox_irls(")]
    cox = doc[doc.index("`cdh_glm_set_survival`"):doc.index("## `locpoly`")]
    assert "Start–stop times and Efron ties are not offered" in cox and "`out5[4]`" in cox


def test_the_instantiations_are_chosen_on_the_host():
    k = open(os.path.join(CSRC, "cox_kernels.hpp")).read()
    for name in ("k_cox_exp<SW>", "k_cox_offsets<true, SW>", "k_cox_scan<1, true, SW>", "k_cox_hazard<SW>",
                 "k_cox_offsets<false, SW>", "k_cox_scan<2, false, SW>", "k_cox_apply<true, SW>", "k_cox_apply<false, SW>"):
        assert name in k, name
    assert "if (h->glm.cox.strata) CHK(chain(std::true_type{})); else CHK(chain(std::false_type{}));" in k
    plan = open(os.path.join(CSRC, "cox_plan.hpp")).read()
    assert "inline void cox_order(" in plan and "inline void cox_order_strata(" in plan
    g = open(os.path.join(CSRC, "glm_kernels.hpp")).read()
    assert "h->glm.cox.strata = false;" in g                    # cdh_glm_set_labels and cdh_glm_set_counts drop them


def test_api_names():
    sig = inspect.signature(cd.CDCoxLoss.__init__).parameters
    assert [(k, v.default, v.kind) for k, v in sig.items()][1:] == [
        ("y", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("X", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("offset", None, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("strata", None, inspect.Parameter.KEYWORD_ONLY), ("weights", None, inspect.Parameter.KEYWORD_ONLY),
        ("device", 0, inspect.Parameter.KEYWORD_ONLY)]
    for prop in ("strata", "weights", "time", "status", "offset"):
        assert isinstance(getattr(cd.CDCoxLoss, prop), property), prop
    for fn in (cd.coxLasso, cd.CoxLassoPath, cd.cvCoxLassoPath):
        p = inspect.signature(fn).parameters
        assert p["strata"].default is None and p["weights"].default is None, fn
        assert "not weighted" in fn.__doc__ or "unweighted penalty scales" in fn.__doc__ or fn is cd.coxLasso
    assert "not weighted by v" in cd.CDCoxLoss.__doc__.replace("NOT", "not")
    assert "strata" not in inspect.signature(cd.coxLambdaMax).parameters and "stratum" in cd.coxLambdaMax.__doc__
    sig = inspect.signature(cd.CDCoxLoss.irls_step).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("apply", True), ("wmin", 1e-5), ("eta_max", 50.0), ("fold", None)]
    assert set(cd.CVPoissonLassoPathResult.__dataclass_fields__) | {"fold_events"} == set(cd.CVCoxLassoPathResult.__dataclass_fields__)


def _problem(n=12):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, 3))
    y = np.c_[rng.exponential(1.0, n), (rng.random(n) < 0.7).astype(float)]
    y[0, 1] = 1.0
    return X, y


def test_refusals_that_precede_the_device():
    n = 12
    X, y = _problem(n)
    g, v = np.arange(n) % 2, np.linspace(0.5, 2.0, n)
    calls = (lambda **kw: cd.CDCoxLoss(y, X, **kw), lambda **kw: cd.coxLasso(X, y, 0.1, **kw),
             lambda **kw: cd.CoxLassoPath(X, y, [0.1], **kw), lambda **kw: cd.cvCoxLassoPath(X, y, [0.1], K=3, **kw))
    for call in calls:
        with pytest.raises(cd.DimensionMismatch, match="strata"):
            call(strata=g[:-1])
        with pytest.raises(cd.DimensionMismatch, match="weights"):
            call(weights=v[:-1])
        with pytest.raises(cd.DimensionMismatch, match="strata"):
            call(strata=np.zeros((n, 1), dtype=int))
        with pytest.raises(cd.ArgumentError, match=r"strata\[3\] is not an integer"):
            call(strata=np.where(np.arange(n) == 3, 0.5, 1.0))
        with pytest.raises(cd.ArgumentError, match=r"strata\[0\] is not an integer"):
            call(strata=np.r_[np.nan, np.ones(n - 1)])
        with pytest.raises(cd.ArgumentError, match=r"strata\[5\] does not fit int32"):
            call(strata=np.where(np.arange(n) == 5, 2 ** 31, 0))
        with pytest.raises(cd.ArgumentError, match="strata must be integers"):
            call(strata=np.array(["a"] * n))
        for bad in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(cd.ArgumentError, match=r"weights\[7\]"):
                call(weights=np.where(np.arange(n) == 7, bad, 1.0))
    # strata or weights together with a loss: they belong to the loss, like the offset
    f = cd.CDCoxLoss.__new__(cd.CDCoxLoss)
    for kw in (dict(strata=g), dict(weights=v)):
        name = list(kw)[0]
        with pytest.raises(cd.ArgumentError, match="%s belongs to the loss" % name):
            cd.coxLasso(f, None, 0.1, **kw)
        with pytest.raises(cd.ArgumentError, match="%s belongs to the loss" % name):
            cd.CoxLassoPath(f, None, [0.1], **kw)
        with pytest.raises(cd.ArgumentError, match="%s belongs to the loss" % name):
            cd.cvCoxLassoPath(f, None, [0.1], K=3, **kw)
    # a fold without weighted events, or holding all of them, before the upload
    yk = y.copy()
    yk[:, 1] = 0.0
    yk[[0, 3], 1] = 1.0                                         # both events in fold 0 of arange % 3
    with pytest.raises(cd.ArgumentError, match="fold 0 holds every event|fold 1 holds no event"):
        cd.cvCoxLassoPath(X, yk, [0.1], K=3, folds=np.arange(n) % 3, strata=g, weights=v)
    yk[1, 1] = 1.0                                              # folds 0 and 1 have events, fold 2 none
    with pytest.raises(cd.ArgumentError, match="fold 2 holds no event"):
        cd.cvCoxLassoPath(X, yk, [0.1], K=3, folds=np.arange(n) % 3, weights=v)


def test_weights_are_normalised_to_sum_to_n_and_strata_become_int32():
    strata, weights = cd.api._strata_weights(np.array([3, -7, 3, 2 ** 31 - 1], dtype=np.int64), [1.0, 2.0, 3.0, 2.0], 4)
    assert strata.dtype == np.int32 and strata.tolist() == [3, -7, 3, 2 ** 31 - 1]
    np.testing.assert_array_equal(weights, np.array([1.0, 2.0, 3.0, 2.0]) * 4 / 8.0)
    assert cd.api._strata_weights(None, None, 4) == (None, None)
    s, _ = cd.api._strata_weights(np.array([1.0, 2.0, -3.0]), None, 3)               # integral floats are integers
    assert s.dtype == np.int32 and s.tolist() == [1, 2, -3]
    _, w = cd.api._strata_weights(None, np.ones(5), 5)
    np.testing.assert_array_equal(w, np.ones(5))                                     # unit weights stay unit weights, bit for bit
