"""Observation weights of the logistic and the Poisson lasso without a GPU: the numpy twin (tests/_glm_weights_numpy.py) against
central differences of the weighted objective, against the same rows replicated, and its fold arithmetic against a fresh
weighted problem on the training rows; the weight check of cdh_glm_set_weights (csrc/glm_plan.hpp) as a stand-alone program
under the host sanitizers; the two new prototypes; the front ends' keywords and the refusals that precede the device."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cv_numpy as CV
import _glm_weights_numpy as GW

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")
U = GW.U
FAMILIES = ("binomial", "poisson")


def _small(family, seed=3):
    """n = 40, p = 6, integer weights 1..3 (normalised), and the replicated rows they stand for."""
    X, y, o, _ = GW.make_data(family, 40, 6, 3, seed)
    reps = np.random.default_rng(seed).integers(1, 4, 40)
    return X, y, o, reps, GW.normalise(reps.astype(np.float64))


# ---- the twin --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_gradient_and_diagonal_against_central_differences(family):
    """d/d beta_j of (1/n) sum v nll by central differences with h = 1e-5: truncation h^2 |F'''| / 6 (|F'''| <= sum v mu |x|^3 / n,
    some hundreds here) and rounding U F / h, together below 1e-7 (1 + |g_j|).  The diagonal by second differences with
    h = 1e-4: truncation h^2 |F''''| / 12 and rounding 4 U F / h^2 = 4e-8 F, together below 1e-5 (1 + d_j)."""
    X, y, o, v = GW.make_data(family, 40, 6, 3, 5, spread=(1e-3, 1e3))
    beta = np.array([0.3, -0.2, 0.0, 0.1, 0.0, -0.4])
    g, d = GW.gradient(family, X, y, o, v, beta, 0.2), GW.diagonal(family, X, y, o, v, beta, 0.2)
    F = lambda b: GW.smooth(family, X, y, o, v, b, 0.2)      # noqa: E731
    eg = ed = 0.0
    for j in range(6):
        e = np.zeros(6)
        e[j] = 1.0
        eg = max(eg, abs((F(beta + 1e-5 * e) - F(beta - 1e-5 * e)) / 2e-5 - g[j]) / (1.0 + abs(g[j])))
        ed = max(ed, abs((F(beta + 1e-4 * e) - 2.0 * F(beta) + F(beta - 1e-4 * e)) / 1e-8 - d[j]) / (1.0 + d[j]))
    print(f"central differences [{family}]: gradient {eg:.1e} diagonal {ed:.1e}")
    assert eg <= 1e-7 and ed <= 1e-5
    # the stored working weight IS the diagonal's weight, and X'W r the gradient, whatever the clamp did
    o_ = GW.rows(family, y, X @ beta + 0.2, o, v, 0.2 if family == "binomial" else 1.0)
    assert o_["clamped"].any() and not o_["clamped"].all()
    np.testing.assert_array_equal(o_["w"], v * o_["w_fam"])
    np.testing.assert_allclose(X.T @ (o_["w"] * o_["r"]) / 40, -g, rtol=0, atol=1e-13 * np.abs(X).max() * np.sum(v))


@pytest.mark.parametrize("family", FAMILIES)
def test_integer_weights_are_replicated_rows(family):
    """v = reps n / N on n = 40 rows against the N = sum reps replicated rows with unit weights: the same objective and
    gradient up to the order of summation -- (N + 64) U times the mean of the terms' magnitudes -- and the same minimiser at
    the solve tolerance of the twins' own tests (1e-8: tests/test_glm_host.py), both solved to optTol 1e-11."""
    X, y, o, reps, v = _small(family)
    Xr, yr, orr = GW.replicate(X, y, o, reps)
    N, ones = len(yr), np.ones(len(yr))
    beta = np.array([0.3, -0.2, 0.0, 0.1, 0.0, -0.4])
    nll_r = GW.rows(family, yr, Xr @ beta, orr, ones, 1e-300, 700.0)["nll"]
    Fw, Fr = GW.smooth(family, X, y, o, v, beta), GW.smooth(family, Xr, yr, orr, ones, beta)
    assert abs(Fw - Fr) <= (N + 64) * U * np.abs(nll_r).mean()
    gw, gr = GW.gradient(family, X, y, o, v, beta), GW.gradient(family, Xr, yr, orr, ones, beta)
    eta = Xr @ beta + (0.0 if orr is None else orr)
    scale = (np.abs(Xr) * (yr + GW.mean(family, eta))[:, None]).mean(axis=0)
    assert np.all(np.abs(gw - gr) <= (N + 64) * U * scale)
    lam = 0.2 * GW.lambda_max(family, X, y, o, v)
    assert abs(lam - 0.2 * GW.lambda_max(family, Xr, yr, orr, ones)) <= 1e-13 * lam
    bw = GW.glm_lasso(family, X, y, o, v, lam, optTol=1e-11)
    br = GW.glm_lasso(family, Xr, yr, orr, ones, lam, optTol=1e-11)
    err = float(np.max(np.abs(bw[0] - br[0])))
    print(f"replication [{family}]: N = {N}, |F_w - F_r| {abs(Fw - Fr):.1e}, max|beta_w - beta_r| {err:.1e}, rounds {bw[2]} / {br[2]}")
    assert bw[3] and br[3] and np.count_nonzero(bw[0]) >= 1 and err <= 1e-8
    on, off, _ = GW.kkt(family, X, y, o, v, bw[0], lam)
    assert on <= 1e-10 and off <= 1e-10


@pytest.mark.parametrize("standardize", (True, False), ids=("std", "raw"))
@pytest.mark.parametrize("intercept", (False, True), ids=("noicpt", "icpt"))
@pytest.mark.parametrize("family", FAMILIES)
def test_fold_scale_is_the_fresh_weighted_problem(family, intercept, standardize):
    """Fold k's problem on the handle -- all n rows, the held-out ones at w = 0, lambda times (V_k / n) / sqrt(n_k / n) (or
    V_k / n), omega of the 0/1 weights -- against a fresh weighted problem on X[train] with its weights renormalised to sum
    to n_k: the same rounds and beta within 1e-12 (the bar of tests/test_cv_logistic_host.py's masked route)."""
    X, y, o, v = GW.make_data(family, 120, 8, 3, 11)
    K, ids = 3, CV.fold_ids(120, 3, 0)
    worst = 0.0
    for k in range(K):
        held = ids == k
        Xt, yt, ot, vt = GW.subset(X, y, o, v, ~held)
        assert abs(vt.sum() - len(yt)) <= 1e-12 * len(yt)
        om = np.sqrt((Xt * Xt).sum(axis=0) / len(yt)) if standardize else None
        lam = 0.2 * GW.lambda_max(family, Xt, yt, ot, vt, om, intercept)
        b, b0, rounds, conv, _ = GW.glm_lasso(family, Xt, yt, ot, vt, lam, om, optTol=1e-11, intercept=intercept)
        mb, mb0, mrounds = GW.masked_lasso(family, X, y, o, v, held, lam, standardize, optTol=1e-11, intercept=intercept)
        assert conv and rounds == mrounds and np.count_nonzero(b) >= 1, (k, rounds, mrounds)
        worst = max(worst, float(np.max(np.abs(b - mb))), abs(b0 - mb0))
    # v = 1: today's factors
    ones = np.ones(120)
    assert GW.fold_scale(ones, ids == 0, True) == pytest.approx(CV.rescale(1.0, int((ids != 0).sum()), 120, True), rel=1e-15)
    assert GW.fold_scale(ones, ids == 0, False) == pytest.approx(CV.rescale(1.0, int((ids != 0).sum()), 120, False), rel=1e-15)
    print(f"fold scale [{family}, intercept {intercept}, standardize {standardize}]: {worst:.2e}")
    assert worst <= 1e-12, worst


def test_record_layouts_and_unit_weights():
    """With v = 1 the weighted rows and records are the unweighted twins', bit for bit; the layouts are 5 and 6 doubles."""
    for family in FAMILIES:
        X, y, o, _ = GW.make_data(family, 50, 4, 2, 1)
        eta = X @ np.array([0.5, -0.3, 0.0, 0.2])
        held = np.arange(50) % 3 == 1
        rec, terms = GW.record(family, y, eta, o, np.ones(50), held, 1e-2, 1.0)
        assert len(rec) == (5 if family == "binomial" else 6) and len(terms) == len(rec)
        if family == "binomial":
            w, z, r, nll, cl = GW.LG.rows(y, eta, 1e-2)
            want = [nll[~held].sum(), w[~held].sum(), cl[~held].sum(), nll[held].sum(), GW.CVL.miss(y, eta)[held].sum()]
        else:
            w, z, r, nll, dev, cl, cp = GW.PN.rows(y, eta, o, 1e-2, 1.0)
            want = [nll[~held].sum(), w[~held].sum(), cl[~held].sum(), cp.sum(), dev[held].sum(), dev[~held].sum()]
        np.testing.assert_allclose(rec, want, rtol=1e-14)
        np.testing.assert_array_equal(GW.rows(family, y, eta, o, np.ones(50), 1e-2, 1.0)["w"], w)


# ---- the weight check ----------------------------------------------------------------------------------------------------------
def test_weight_check_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "glm_weights_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, os.path.join(HERE, "glm_weights_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert re.search(r"^glm_weights_main OK \d+$", out.strip()), out
    assert int(out.split()[-1]) >= 200                      # (5 lengths x (1 + 18 good + 21 to 42 bad) cases, and n = 0)


# ---- the prototypes ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = (("cdh_glm_set_weights", 2), ("cdh_glm_get_weights", 2))


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
    # the step exports keep their signatures; the weighted instantiations are chosen on the host
    assert [len(getattr(L, n).argtypes) for n in ("cdh_glm_irls", "cdh_glm_irls_fold", "cdh_glm_poisson_irls")] == [4, 5, 6]
    k = open(os.path.join(CSRC, "glm_kernels.hpp")).read()
    for fam in ("GlmBinomial", "GlmPoisson"):
        assert re.search(r"struct %s \{[^}]*kWeights = false" % fam, k), fam
    for fam in ("GlmBinomialFoldW : GlmBinomialFold", "GlmPoissonW : GlmPoisson"):
        assert re.search(r"struct %s \{\s*static constexpr bool kWeights = true;" % fam, k), fam
    assert "if constexpr (F::kWeights)" in k and "h->glm.weighted = false;" in k
    assert "glm_step<GlmBinomialFoldW>(h, -1," in src and "glm_step<GlmPoissonW>(h, k," in src
    plan = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "glm_plan.hpp")).read())
    assert "inline int64_t glm_first_bad_weight(" in plan


def test_api_names():
    kw = inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(cd.CDLogisticLoss.__init__).parameters
    assert [(k, v.default, v.kind) for k, v in sig.items()][3:] == [("weights", None, kw), ("device", 0, kw)]
    sig = inspect.signature(cd.CDPoissonLoss.__init__).parameters
    assert list(sig)[1:4] == ["y", "X", "offset"]
    assert [(k, v.default, v.kind) for k, v in sig.items()][4:] == [("weights", None, kw), ("device", 0, kw)]
    for cls in (cd.CDLogisticLoss, cd.CDPoissonLoss):
        assert isinstance(cls.weights, property) and "not weighted by v" in cls.__doc__.replace("NOT", "not")
    for fn in (cd.logisticLasso, cd.LogisticLassoPath, cd.cvLogisticLassoPath, cd.poissonLasso, cd.PoissonLassoPath,
               cd.cvPoissonLassoPath):
        p = inspect.signature(fn).parameters["weights"]
        assert p.default is None and p.kind == kw, fn
    for fn in (cd.logisticLambdaMax, cd.poissonLambdaMax):
        assert "weights" not in inspect.signature(fn).parameters and "observation weights" in fn.__doc__


# ---- the refusals that precede the device ------------------------------------------------------------------------------------------
def test_refusals_that_precede_the_device():
    n = 12
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, 3))
    yb, yp = (np.arange(n) % 2).astype(float), rng.poisson(1.0, n).astype(float) + 1.0
    v = np.linspace(0.5, 2.0, n)
    calls = []
    for icpt in (False, True):
        calls += [lambda icpt=icpt, **kw: cd.logisticLasso(X, yb, 0.1, fit_intercept=icpt, **kw),
                  lambda icpt=icpt, **kw: cd.LogisticLassoPath(X, yb, [0.1], fit_intercept=icpt, **kw),
                  lambda icpt=icpt, **kw: cd.cvLogisticLassoPath(X, yb, [0.1], K=3, fit_intercept=icpt, **kw),
                  lambda icpt=icpt, **kw: cd.poissonLasso(X, yp, 0.1, fit_intercept=icpt, **kw),
                  lambda icpt=icpt, **kw: cd.PoissonLassoPath(X, yp, [0.1], fit_intercept=icpt, **kw),
                  lambda icpt=icpt, **kw: cd.cvPoissonLassoPath(X, yp, [0.1], K=3, fit_intercept=icpt, offset=np.zeros(n), **kw)]
    calls += [lambda **kw: cd.CDLogisticLoss(yb, X, **kw), lambda **kw: cd.CDPoissonLoss(yp, X, **kw),
              lambda **kw: cd.CDPoissonLoss(yp, X, np.zeros(n), **kw)]
    for call in calls:
        with pytest.raises(cd.DimensionMismatch, match="weights"):
            call(weights=v[:-1])
        with pytest.raises(cd.DimensionMismatch, match="weights"):
            call(weights=np.ones((n, 1)))
        for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
            with pytest.raises(cd.ArgumentError, match=r"weights\[7\] is not finite and > 0"):
                call(weights=np.where(np.arange(n) == 7, bad, 1.0))
    # weights together with a loss: they belong to the loss, like the offset
    for cls, fns in ((cd.CDLogisticLoss, (cd.logisticLasso, cd.LogisticLassoPath, cd.cvLogisticLassoPath)),
                     (cd.CDPoissonLoss, (cd.poissonLasso, cd.PoissonLassoPath, cd.cvPoissonLassoPath))):
        f = cls.__new__(cls)                  # (an object made without a device)
        f.n = n
        for fn in fns:
            lam = 0.1 if fn in (cd.logisticLasso, cd.poissonLasso) else [0.1]
            with pytest.raises(cd.ArgumentError, match="weights belongs to the loss"):
                fn(f, None, lam, weights=v)


def test_starts_with_weights():
    """logit(sum vy / sum v) and log(sum vy / sum v e^o); without weights the calls of before, bit for bit."""
    y = np.array([0.0, 1.0, 1.0, 0.0, 1.0])
    v = np.array([2.0, 0.5, 0.5, 1.0, 1.0])
    o = np.log(np.array([1.0, 2.0, 0.5, 1.0, 3.0]))
    ybar = (v * y).sum() / v.sum()
    assert cd.api._logit_start(y, v) == float(np.log(ybar / (1.0 - ybar)))
    assert cd.api._logit_start(y) == float(np.log(np.mean(y) / (1.0 - np.mean(y))))
    assert cd.api._logit_start(y, np.ones(5)) == pytest.approx(cd.api._logit_start(y), rel=1e-15)
    assert cd.api._poisson_start(y, o, v) == float(np.log((v * y).sum() / (v * np.exp(o)).sum()))
    assert cd.api._poisson_start(y, None, v) == float(np.log((v * y).sum() / v.sum()))
    assert cd.api._poisson_start(y, o) == float(np.log(y.sum() / np.exp(o).sum()))
    assert cd.api._poisson_start(y) == float(np.log(y.sum() / 5.0))
    assert cd.api._poisson_start(y, o, v) == pytest.approx(GW.null_intercept("poisson", y, o, v), rel=1e-15)
    assert cd.api._logit_start(y, v) == pytest.approx(GW.null_intercept("binomial", y, None, v), rel=1e-15)
    with pytest.raises(cd.ArgumentError, match="both kinds"):
        cd.api._logit_start(np.ones(5), v)
    with pytest.raises(cd.ArgumentError, match="positive count"):
        cd.api._poisson_start(np.zeros(5), o, v)
