"""Efron ties of the Cox lasso without a GPU: the twin's two halves (tests/_cox_efron_numpy.py) against each other by central
differences and against closed forms; the two new prototypes -- declared, bound with the right arity, cited, guarded, in the
Julia binding and in INTEGRATION.md; the front ends' ties keyword and the refusals that precede the device."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_efron_numpy as CE
import _cox_strata_numpy as CS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")

NEW_SYMBOLS = (("cdh_glm_set_cox_ties", 2), ("cdh_glm_get_cox_ties", 2))


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def _forty():
    """About 40 rows with rounded times (heavy ties), weights and two strata."""
    rng = np.random.default_rng(11)
    n = 40
    t = np.ceil(2.0 * rng.exponential(1.0, n)) / 2.0             # rounded up to halves: groups of several events
    status = (rng.random(n) < 0.7).astype(np.float64)
    g = rng.integers(0, 2, n)
    v = rng.uniform(0.25, 4.0, n)
    eta = rng.normal(0.0, 0.7, n)
    order, first, last, _, _ = CS.groups(t, g)
    tied_events = max(int(status[order][first[s]:last[s] + 1].sum()) for s in range(n))
    assert tied_events >= 3                                      # the data do exercise l >= 2
    return n, t, status, g, v, eta


def test_the_step_d_is_the_gradient_of_the_nll_half():
    """d = dv - ev A of the step half against central differences of the definition half, eta by eta."""
    n, t, status, g, v, eta = _forty()
    q = CE.rows(eta, None, t, status, 1e-300, 700.0, strata=g, weights=v)
    h = 1e-5
    for i in range(n):
        e = np.zeros(n)
        e[i] = h
        num = (CE.npl(eta + e, t, status, g, v) - CE.npl(eta - e, t, status, g, v)) / (2 * h)
        assert abs(-q["d"][i] - num) <= 2e-8 * max(1.0, abs(num)), (i, q["d"][i], num)


def test_w_raw_is_the_derivative_of_d():
    """w_raw = ev A - ev^2 B is the diagonal of the Hessian: minus the central difference of d_i in eta_i."""
    n, t, status, g, v, eta = _forty()
    q = CE.rows(eta, None, t, status, 1e-300, 700.0, strata=g, weights=v)
    h = 1e-5
    for i in range(n):
        e = np.zeros(n)
        e[i] = h
        dp = CE.rows(eta + e, None, t, status, 1e-300, 700.0, strata=g, weights=v)["d"][i]
        dm = CE.rows(eta - e, None, t, status, 1e-300, 700.0, strata=g, weights=v)["d"][i]
        num = -(dp - dm) / (2 * h)
        assert abs(q["w_raw"][i] - num) <= 2e-8 * max(1.0, abs(num)), (i, q["w_raw"][i], num)


def test_the_record_of_the_step_is_the_nll_half():
    n, t, status, g, v, eta = _forty()
    for train in (None, np.arange(n) % 3 != 1):
        q = CE.rows(eta, None, t, status, 1e-300, 700.0, train, strata=g, weights=v)
        want = CE.npl(eta, t, status, g, v, train)
        assert abs(math.fsum(q["nll"]) - want) <= 1e-12 * abs(want)
        ql = CE.rows(eta, None, t, status, 1e-300, 700.0, train, strata=g, weights=v, dtype=np.longdouble)
        for key in ("w_raw", "d", "A", "B"):
            np.testing.assert_allclose(q[key], ql[key], rtol=1e-12, atol=1e-300)


def test_closed_forms():
    # eta = 0, unit weights, times [1, 1, 1, 2], status [1, 1, 0, 1]: log 4 + log 3 + log 1 = log 12 (Breslow: log 16)
    t, s = np.array([1.0, 1.0, 1.0, 2.0]), np.array([1.0, 1.0, 0.0, 1.0])
    z = np.zeros(4)
    assert abs(CE.npl(z, t, s) - math.log(12.0)) <= 1e-15
    assert abs(math.fsum(CE.rows(z, None, t, s, 1e-300, 700.0)["nll"]) - math.log(12.0)) <= 4e-16 * math.log(12.0) * 4
    assert abs(CS.npl(z, t, s) - math.log(16.0)) <= 1e-15
    # all n rows tied and all events, eta = 0: den_l = n - l, n nll = log n!
    for n in (1, 2, 7, 40):
        t, s, z = np.ones(n), np.ones(n), np.zeros(n)
        want = math.lgamma(n + 1)
        assert abs(CE.npl(z, t, s) - want) <= 1e-13 * max(want, 1.0)
        assert abs(math.fsum(CE.rows(z, None, t, s, 1e-300, 700.0)["nll"]) - want) <= 1e-13 * max(want, 1.0)


def test_without_tied_events_it_is_the_breslow_twin():
    """Distinct times (and tied times of which at most one is an event): every d is 1, m = dv, den = S."""
    rng = np.random.default_rng(5)
    n = 40
    t = rng.permutation(n).astype(np.float64)
    t[1::4] = t[0::4]                                            # pairs of tied times ...
    status = (rng.random(n) < 0.7).astype(np.float64)
    status[1::4] = 0.0                                           # ... whose second row is censored
    g, v = rng.integers(0, 2, n), rng.uniform(0.25, 4.0, n)
    eta = rng.normal(0.0, 0.7, n)
    e = CE.rows(eta, None, t, status, 1e-5, 50.0, strata=g, weights=v)
    b = CS.rows(eta, np.zeros(n), t, status, 1e-5, 50.0, strata=g, weights=v)
    for key in ("w", "z", "r", "d", "A", "B", "S"):
        np.testing.assert_allclose(e[key], b[key], rtol=64 * 2.0 ** -53, atol=0.0, err_msg=key)
    assert abs(math.fsum(e["nll"]) - math.fsum(b["nll"])) <= 1e-13 * abs(math.fsum(b["nll"]))
    assert abs(CE.npl(eta, t, status, g, v) - CS.npl(eta, t, status, g, v)) <= 1e-13 * abs(CS.npl(eta, t, status, g, v))
    np.testing.assert_array_equal(e["rho"], 1.0)


# ---- the prototypes ------------------------------------------------------------------------------------------------------------
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
    before = hdr[: hdr.index("int32_t cdh_glm_set_cox_ties(")]
    assert "coxph's convention" in before[before.rindex("/*"):]                      # which convention the weights follow
    jl = open(os.path.join(ROOT, "julia", "CoordinateDescentHIP.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in NEW_SYMBOLS:
        assert "(:%s, libcdhip)" % name in jl, name
        assert "`%s`" % name in doc, name
    assert "ties::Symbol=:breslow" in jl
    assert len(L.cdh_glm_cox_irls.argtypes) == 6                                      # the step keeps its signature
    for text in (hdr, open(os.path.join(ROOT, "README.md")).read(), doc):
        assert "Efron ties are offered for right-censored data; not yet with start" in " ".join(text.replace(" * ", " ").split())


def test_the_kernels_live_in_a_second_translation_unit():
    """cdhip.hip instantiates no Efron kernel: they are cox_efron.hip's, the host body is included last, and the build
    compiles both files into the one library."""
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    unit = open(os.path.join(CSRC, "cox_efron.hip")).read()
    host = open(os.path.join(CSRC, "cox_efron_host.hpp")).read()
    assert src.index('#include "cox_interval.hpp"') < src.index('#include "cox_efron_host.hpp"')
    assert src.rindex("#include") == src.index('#include "cox_efron_host.hpp"')
    for k in ("k_efron_mark", "k_efron_hazard", "k_efron_apply"):
        assert "void %s(" % k in unit
        assert k not in re.sub(r"//[^\n]*", "", host) and k not in re.sub(r"//[^\n]*", "", src)
    code = re.sub(r"//[^\n]*", "", unit)
    assert "#pragma clang fp contract(off)" in code
    assert not re.search(r"atomic|cooperative|__threadfence|while\s*\(\s*(?:true|1)\s*\)|volatile|asm", code)
    lib = open(os.path.join(ROOT, "coordinatedescent.jl_amd", "_lib.py")).read()
    assert '"cdhip.hip"' in lib and '"cox_efron.hip"' in lib
    k = open(os.path.join(CSRC, "cox_kernels.hpp")).read()
    assert "if (h->glm.cox.efron) CHK(cox_launch_efron(h, k, apply, pm));" in k
    g = open(os.path.join(CSRC, "glm_kernels.hpp")).read()
    assert "h->glm.cox.efron = false;" in g                     # cdh_glm_set_labels and cdh_glm_set_counts drop the rule


# ---- the front ends ------------------------------------------------------------------------------------------------------------
def test_api_names_and_defaults():
    assert callable(cd.CDCoxLoss.set_ties) and isinstance(cd.CDCoxLoss.ties, property)
    assert list(inspect.signature(cd.CDCoxLoss.set_ties).parameters) == ["self", "ties"]
    for fn in (cd.coxLasso, cd.CoxLassoPath, cd.cvCoxLassoPath):
        p = inspect.signature(fn).parameters
        assert p["ties"].default == "breslow", fn
        assert "ties" in fn.__doc__
    assert "ties" not in inspect.signature(cd.CDCoxLoss.__init__).parameters
    assert "ties" not in inspect.signature(cd.CDCoxLoss.irls_step).parameters
    assert "ties" not in cd.CVCoxLassoPathResult.__dataclass_fields__
    assert "no Efron" not in cd.CDCoxLoss.__doc__ and 'set_ties("efron")' in cd.CDCoxLoss.__doc__


def test_refusals_that_precede_the_device():
    rng = np.random.default_rng(0)
    n = 12
    X = rng.standard_normal((n, 3))
    y = np.c_[rng.exponential(1.0, n), (rng.random(n) < 0.7).astype(float)]
    y[0, 1] = 1.0
    y3 = np.c_[np.zeros(n), y[:, 0] + 1.0, y[:, 1]]
    calls = (lambda yy, **kw: cd.coxLasso(X, yy, 0.1, **kw), lambda yy, **kw: cd.CoxLassoPath(X, yy, [0.1], **kw),
             lambda yy, **kw: cd.cvCoxLassoPath(X, yy, [0.1], K=3, **kw))
    for call in calls:
        for bad in ("exact", "Efron", None, 1):
            with pytest.raises(cd.ArgumentError, match="ties must be"):
                call(y, ties=bad)
        with pytest.raises(cd.ArgumentError, match="Efron ties are not offered with start-stop times"):
            call(y3, ties="efron")
    # a loss that was passed in: the keyword must name the loss's own rule
    f = cd.CDCoxLoss.__new__(cd.CDCoxLoss)
    assert f.ties == "breslow"                                   # (no handle: the default)
    for call in (lambda **kw: cd.coxLasso(f, None, 0.1, **kw), lambda **kw: cd.CoxLassoPath(f, None, [0.1], **kw),
                 lambda **kw: cd.cvCoxLassoPath(f, None, [0.1], K=3, **kw)):
        with pytest.raises(cd.ArgumentError, match='ties="efron" disagrees with the loss'):
            call(ties="efron")
        with pytest.raises(cd.ArgumentError, match="ties must be"):
            call(ties="exact")
    with pytest.raises(cd.ArgumentError, match="ties must be"):
        f.set_ties("exact")
    f._interval = True
    with pytest.raises(cd.ArgumentError, match="Efron ties are not offered with start-stop times"):
        f.set_ties("efron")
    with pytest.raises(cd.ArgumentError, match="Efron ties are not offered with start-stop times"):
        cd.coxLasso(f, None, 0.1, ties="efron")
