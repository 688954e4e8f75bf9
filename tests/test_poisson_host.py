"""The Poisson lasso without a GPU: the numpy twin (tests/_poisson_numpy.py: IRLS over the CPU oracle's weighted lasso, the
offset outside the working response) against an independent solver -- scipy's L-BFGS-B on the split beta = beta+ - beta- with
bounds, started from zero -- and against the KKT conditions of the objective; the twin's row formulas at their extremes; the
record's length in the header the kernel and the host share (a new probe, tests/poisson_plan_main.cpp); the front end's
refusals that precede the device; and the three new prototypes."""
import os
import re
import subprocess

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _glm_plan as GP
import _poisson_numpy as PN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")

_TWIN = {}


def twin_path(seed):
    """The twin's warm-started path of a data set at lambda / lambda_max in PN.FRACS, computed once and shared."""
    if seed not in _TWIN:
        X, y, o, _ = PN.make_data(seed)
        icpt = PN.DATASETS[seed][3]
        lmax = PN.lambda_max(X, y, o, intercept=icpt)
        lams = [fr * lmax for fr in PN.FRACS]
        _TWIN[seed] = (X, y, o, icpt, lams, PN.poisson_path(X, y, o, lams, standardize=False, intercept=icpt))
    return _TWIN[seed]


def lbfgs(X, y, o, lam, icpt):
    """min F over (beta+, beta-, b0) >= (0, 0, free) from zero -> (beta, b0, F): no IRLS, no coordinate descent, no oracle."""
    from scipy.optimize import minimize
    n, p = X.shape

    def fg(v):
        bp, bm, b0 = v[:p], v[p:2 * p], (v[2 * p] if icpt else 0.0)
        eta = X @ (bp - bm) + b0 + o
        mu = np.exp(eta)
        g = X.T @ (mu - y) / n
        grad = np.r_[g + lam, -g + lam, [np.sum(mu - y) / n] if icpt else []]
        return np.mean(mu - y * eta) + lam * np.sum(bp + bm), grad

    m = 2 * p + (1 if icpt else 0)
    res = minimize(fg, np.zeros(m), jac=True, method="L-BFGS-B", bounds=[(0.0, None)] * (2 * p) + [(None, None)] * (m - 2 * p),
                   options=dict(maxiter=100000, maxfun=1000000, ftol=1e-17, gtol=1e-13, maxcor=40))
    beta = res.x[:p] - res.x[p:2 * p]
    b0 = float(res.x[2 * p]) if icpt else 0.0
    return beta, b0, PN.objective(X, y, o, beta, lam, None, b0)


@pytest.mark.parametrize("seed", sorted(PN.DATASETS))
def test_twin_against_lbfgsb(seed):
    """F_twin <= F_lbfgs + 1e-12 and max |beta_twin - beta_lbfgs| <= 1e-6 (the second is L-BFGS-B's own stopping accuracy);
    every solve of the path converges within 25 rounds, monotone.  Measured when this was written: F differences within
    +-2e-16, beta within 9.2e-10, 4 to 5 rounds."""
    X, y, o, icpt, lams, path = twin_path(seed)
    for lam, (b, b0, rounds, conv, rise) in zip(lams, path):
        lb, lb0, F_l = lbfgs(X, y, o, lam, icpt)
        F_t = PN.objective(X, y, o, b, lam, None, b0)
        err = max(float(np.max(np.abs(b - lb))), abs(b0 - lb0))
        print(f"twin vs L-BFGS-B seed {seed} lam {lam:.4f}: F_twin - F_lbfgs {F_t - F_l:+.1e}, beta {err:.1e}, {rounds} rounds, "
              f"rise {rise:.1e}, nnz {np.count_nonzero(b)}")
        assert conv and rounds <= 25 and rise <= 1e-10 * max(1.0, abs(F_t))
        assert F_t <= F_l + 1e-12
        assert err <= 1e-6
    assert np.count_nonzero(path[-1][0]) > np.count_nonzero(path[0][0]) >= 1


@pytest.mark.parametrize("seed", sorted(PN.DATASETS))
def test_twin_kkt(seed):
    """The KKT conditions of F itself at the twin's solutions.  IRLS stops at a step below optTol = 1e-7; the Newton step's
    quadratic convergence leaves the gradient far below, and the inner solves stop at 1e-12: the slack is 1e3 optTol^2 + 1e2
    inner optTol = 1.1e-10, the binomial test's 1e-10 tied to the same two tolerances.  Measured when this was written: <= 4.7e-13."""
    X, y, o, icpt, lams, path = twin_path(seed)
    slack = 1e3 * 1e-7 ** 2 + 1e2 * 1e-12
    for lam, (b, b0, rounds, conv, _) in zip(lams, path):
        on, off, ic = PN.kkt(X, y, o, b, lam, None, b0)
        print(f"twin KKT seed {seed} lam {lam:.4f}: on {on:.1e} off {off:.1e} intercept {ic:.1e}, {rounds} rounds")
        assert conv and on <= slack and off <= slack
        if icpt:
            assert ic <= slack and abs(b0) > 0.05


def test_twin_rows_at_the_extremes():
    """The per-row formulas where naive ones fail: nothing overflows at |eta| = 745, eta is capped strictly above eta_max,
    y = 0 has dev = 2 mu exactly without a log(0), y = mu has dev = 0 and r = 0, and a mean below wmin clamps only the weight."""
    wmin, emax = 1e-5, 50.0
    #                 +745   -745   +emax  -emax  y = 0  y = mu        mu < wmin  just above the cap
    eta = np.array([745.0, -745.0, emax, -emax, 1.25, np.log(8.0), -20.0, np.nextafter(emax, 100.0)])
    y = np.array([3.0, 0.0, 2.0, 1.0, 0.0, 0.0, 4.0, 7.0])
    y[5] = np.exp(eta[5])
    for o in (None, np.zeros(8)):
        w, z, r, nll, dev, cl, cap = PN.rows(y, eta, o, wmin, emax)
        for v in (w, z, r, nll, dev):
            assert np.isfinite(v).all(), v
        assert cap.tolist() == [True, False, False, False, False, False, False, True]
        assert cl.tolist() == [False, True, False, True, False, False, True, False]
        assert w[0] == np.exp(emax) and w[2] == np.exp(emax) and w[7] == np.exp(emax)
        assert (w[[1, 3, 6]] == wmin).all() and (w >= wmin).all()
        assert dev[1] == 2.0 * np.exp(-745.0) and r[1] == -np.exp(-745.0) / wmin      # y = 0 at a denormal mean
        assert dev[4] == 2.0 * np.exp(1.25) and nll[4] == np.exp(1.25) and r[4] == -1.0
        assert dev[5] == 0.0 and r[5] == 0.0 and z[5] == eta[5]
        assert r[6] == (4.0 - np.exp(-20.0)) / wmin and z[6] == eta[6] + r[6]           # only w is clamped: d stays y - mu
        assert nll[0] == np.exp(emax) - 3.0 * emax                                       # the capped eta, not 745
    # the offset moves mu, never the stored working response: z - r is eta_lin whatever o is
    o = np.array([-745.0, 700.0, 1.0, 10.0, -1.25, 0.5, 20.0, -1.0])
    w, z, r, nll, dev, cl, cap = PN.rows(y, eta, o, wmin, emax)
    assert np.isfinite(np.r_[w, z, r, nll, dev]).all()
    assert w[0] == 1.0 and w[4] == 1.0 and cap.tolist() == [False] * 2 + [True] + [False] * 5
    assert np.all(np.abs((z - r) - eta) <= 2 * PN.U * (np.abs(eta) + 2 * np.abs(r)))     # two roundings, of z and of z - r
    # a positive count at a mean so small that y / mu overflows: the formula's deviance is +inf, never NaN, and w, z, r and
    # nll stay finite (the true deviance, 2 y (log y + 745) - 2 y, is finite; means that small are not fitted)
    with np.errstate(over="ignore"):
        w, z, r, nll, dev, _, _ = PN.rows([1.0], [-745.0], None, wmin, emax)
    assert dev[0] == np.inf and np.isfinite(np.r_[w, z, r, nll]).all()


# ---- the record ----------------------------------------------------------------------------------------------------------------
def test_record_length_in_the_shared_header(tmp_path):
    """kGlmPoisVals = 6, and 6 records of the largest grid fit the sums' buffer as the handle sizes it at its smallest."""
    exe = str(tmp_path / "poisson_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, os.path.join(HERE, "poisson_plan_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "poisson_plan_main" and out[1] == "OK"
    vals, max_grid, fold_vals = (int(v) for v in out[2:5])
    assert vals == 6 and max_grid == GP.MAX_GRID and fold_vals == 5
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    assert "kGlmMaxGrid * kGlmPoisVals" in src                # the static_assert beside partials_doubles


# ---- the front end -----------------------------------------------------------------------------------------------------------
def test_refusals_that_precede_the_device():
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((12, 3)), rng.poisson(1.0, 12).astype(float)
    with pytest.raises(TypeError):
        cd.CDPoissonLoss(y, X.astype(np.float32))
    with pytest.raises(cd.DimensionMismatch):
        cd.CDPoissonLoss(y[:11], X)
    with pytest.raises(cd.DimensionMismatch):
        cd.CDPoissonLoss(y, X, np.zeros(11))
    for cls in (cd.CDLeastSquaresLoss, cd.CDWeightedLSLoss, cd.CDQuadraticLoss, cd.CDLogisticLoss):
        f = cls.__new__(cls)                  # (objects made without a device)
        with pytest.raises(TypeError):
            cd.poissonLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1))
        with pytest.raises(TypeError):
            cd.poissonLambdaMax(f)
        with pytest.raises(TypeError):
            cd.poissonLasso(f, None, 0.1)
        with pytest.raises(TypeError):
            cd.cvPoissonLassoPath(f, None, [0.1], K=3)
    f = cd.CDPoissonLoss.__new__(cd.CDPoissonLoss)
    with pytest.raises(TypeError):                              # a sibling, not a subclass: the binomial loop keeps refusing it
        cd.logisticLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1))
    with pytest.raises(TypeError):
        cd.logisticLambdaMax(f)
    with pytest.raises(cd.ArgumentError, match="warmStart"):
        cd.poissonLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1), cd.CDOptions(warmStart=False))
    with pytest.raises(cd.ArgumentError, match="column of ones"):
        cd.poissonLasso(f, None, 0.1, fit_intercept=True)
    with pytest.raises(cd.ArgumentError, match="belongs to the loss"):
        cd.poissonLasso(f, None, 0.1, offset=np.zeros(12))
    # no positive count: the null model's intercept is -infinity, refused before the upload
    for call in (lambda: cd.poissonLasso(X, np.zeros(12), 0.1, fit_intercept=True),
                 lambda: cd.PoissonLassoPath(X, np.zeros(12), [0.1], fit_intercept=True),
                 lambda: cd.cvPoissonLassoPath(X, np.zeros(12), [0.1], K=3, fit_intercept=True)):
        with pytest.raises(cd.ArgumentError, match="positive count"):
            call()
    yk = y.copy()
    yk[np.arange(12) % 3 != 1] = 0.0                            # the training rows of fold 1 hold no count
    yk[1] = 2.0
    with pytest.raises(cd.ArgumentError, match="positive count"):
        cd.cvPoissonLassoPath(X, yk, [0.1], K=3, folds=np.arange(12) % 3, fit_intercept=True)
    with pytest.raises(cd.ArgumentError, match="measure"):
        cd.cvPoissonLassoPath(X, y, [0.1], K=3, measure="mse")
    with pytest.raises(cd.ArgumentError, match="empty"):
        cd.cvPoissonLassoPath(X, y, [], K=3)
    o = cd.IRLSOptions()
    assert (o.maxIter, o.optTol, o.wmin, o.etaMax) == (25, 1e-7, 1e-5, 50.0)


NEW_SYMBOLS = (("cdh_glm_set_counts", 3), ("cdh_glm_get_offset", 2), ("cdh_glm_poisson_irls", 6))


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
    for n in ("CDPoissonLoss", "poissonLasso_", "poissonLasso", "poissonLambdaMax", "PoissonLassoPath", "PoissonLassoSolution",
              "PoissonLassoPathResult", "cvPoissonLassoPath", "CVPoissonLassoPathResult"):
        assert hasattr(cd, n), n
    assert issubclass(cd.CDPoissonLoss, cd.CDWeightedLSLoss) and not issubclass(cd.CDPoissonLoss, cd.CDLogisticLoss)
    assert isinstance(cd.CDPoissonLoss.counts, property) and isinstance(cd.CDPoissonLoss.offset, property)
    assert hasattr(cd.CDPoissonLoss, "irls_step") and hasattr(cd.CDPoissonLoss, "objective")
    fields = set(cd.CVLogisticLassoPathResult.__dataclass_fields__) - {"fold_class"}
    assert set(cd.CVPoissonLassoPathResult.__dataclass_fields__) == fields
    for fld in ("nll", "deviance", "rounds", "converged", "monotone", "capped", "intercept", "held_deviance"):
        assert fld in cd.PoissonLassoSolution.__dataclass_fields__, fld
    # the kernel is plain C++ with contraction off in the row function, and the binomial family argument stays closed
    k = open(os.path.join(CSRC, "glm_kernels.hpp")).read()
    row = k[k.index("PoisRow pois_row("):k.index("template <class F, bool APPLY>", k.index("PoisRow pois_row("))]
    assert "#pragma clang fp contract(off)" in row and "asm" not in row
    assert 'if (family != 0) return fail(h, CDH_BAD_ARG, "unknown family' in k
