"""The logistic lasso without a GPU: the host arithmetic of cdh_glm_irls (csrc/glm_plan.hpp) as a stand-alone program under the
host sanitizers and against its Python restatement (tests/_glm_plan.py); the numpy twin (tests/_logistic_numpy.py: IRLS over the
CPU oracle's weighted lasso) against scikit-learn's liblinear and against the KKT conditions of the objective; the transition
the residual's state gained for a step that rewrites r (a new shim, tests/resid_glm_shim.cpp); the front end's refusals that
precede the device; and the three new prototypes."""
import ctypes as C
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
import _glm_plan as GP
import _logistic_numpy as LG

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")


# ---- the plan ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glm") / "glm_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "glm_plan_main.cpp")], check=True)
    return exe


def test_plan_covers_every_row_once(plan_exe):
    """n = 1 .. 600 and around every constant of the plan: [0, n) and the pad rows exactly once, records == grid."""
    out = subprocess.run([plan_exe], check=True, capture_output=True, text=True).stdout
    assert "glm_plan_main OK rows=512" in out, out


def test_python_restatement_matches_the_header(plan_exe):
    cases = [(n, cap) for cap in (GP.MAX_GRID, 1, 2, 3, 0, 5000)
             for n in list(range(1, 70)) + [511, 512, 513, 1023, 1024, 1025, 1536, 1537, 524287, 524288, 524289, 2000000]]
    args = [str(v) for n, cap in cases for v in (GP.padded(n), cap)]
    lines = subprocess.run([plan_exe] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    for (n, cap), line in zip(cases, lines):
        ld, _, vecs, tiles, grid, records, strides = (int(v) for v in line.split())
        assert GP.plan(n, cap) == dict(ld=ld, vecs=vecs, tiles=tiles, grid=grid, records=records, strides=strides), (n, cap)
    assert GP.plan(524288)["strides"] == 1 and GP.plan(524289)["strides"] == 2 and GP.plan(1025, 2)["strides"] == 2


def test_plan_header_holds_no_hip():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "glm_plan.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|hip[A-Z_]|threadIdx|blockIdx", code)


# ---- the twin ----------------------------------------------------------------------------------------------------------------
CASES = ((257, 20, 3, 1), (500, 50, 5, 2))
FRACS = (0.5, 0.1)
ICPT = (300, 12, 3, 7, 0.8)           # n, p, s, seed, intercept
_TWIN = {}


def twin(n, p, s, seed, frac, intercept=None):
    """The twin's solution of a case, computed once and shared."""
    key = (n, p, s, seed, frac, intercept)
    if key not in _TWIN:
        X, y, _ = LG.make_data(n, p, s, seed, intercept or 0.0)
        lam = frac * LG.lambda_max(X, y, intercept=intercept is not None)
        beta, b0, rounds, conv, rise = LG.logistic_lasso(X, y, lam, optTol=1e-11, intercept=intercept is not None)
        _TWIN[key] = (X, y, lam, beta, b0, rounds, conv, rise)
    return _TWIN[key]


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("n,p,s,seed", CASES)
def test_twin_against_liblinear(n, p, s, seed, frac):
    """Measured when this was written: 7.5e-13, 1.0e-12, 1.1e-12 and 2.1e-10.  Smaller lambda is left out on purpose:
    liblinear stops short there (1.6e-8 at (2000, 40), 0.02 lambda_max)."""
    from sklearn.linear_model import LogisticRegression
    X, y, lam, beta, _, rounds, conv, rise = twin(n, p, s, seed, frac)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # (liblinear reports its iteration limit at tol = 1e-12: the bound below is the check)
        # random_state pins liblinear's shuffle: at (500, 50), 0.1 lambda_max its answer moves between 1e-10 and 9.9e-9 of the
        # twin with the seed (seeds 0 .. 2 and the global generator tried), whatever max_iter is -- its own floor, under the bound
        sk = LogisticRegression(penalty="l1", solver="liblinear", fit_intercept=False, C=1.0 / (lam * n), tol=1e-12,
                                random_state=0).fit(X, y)
    err = float(np.max(np.abs(sk.coef_.ravel() - beta)))
    print(f"twin vs liblinear ({n}, {p}) {frac}: {err:.2e}, {rounds} rounds, rise {rise:.1e}")
    assert conv and np.count_nonzero(beta) >= 1
    assert err <= 1e-8, err


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("n,p,s,seed,icpt", [c + (None,) for c in CASES] + [ICPT])
def test_twin_kkt(n, p, s, seed, icpt, frac):
    """Measured when this was written: <= 5e-14."""
    X, y, lam, beta, b0, rounds, conv, rise = twin(n, p, s, seed, frac, icpt)
    on, off, ic = LG.kkt(X, y, beta, lam, None, b0)
    print(f"twin KKT ({n}, {p}) {frac}: on {on:.1e} off {off:.1e} intercept {ic:.1e}, {rounds} rounds")
    assert conv and rounds <= 12 and rise <= 1e-10
    assert on <= 1e-10 and off <= 1e-10
    if icpt is not None:
        assert ic <= 1e-10 and abs(b0) > 0.1


def test_twin_rows_at_the_extremes():
    """The per-row formulas where the naive ones fail: p and q never round to a difference, w clamps, nothing overflows."""
    eta = np.array([0.0, 40.0, -40.0, 800.0, -800.0, 1e-300])
    y = np.array([1.0, 0.0, 1.0, 1.0, 0.0, 0.25])
    w, z, r, nll, cl = LG.rows(y, eta, 1e-5)
    assert w[0] == 0.25 and r[0] == 2.0 and nll[0] == np.log1p(1.0) and not cl[0]
    assert cl[1:5].all() and (w[1:5] == 1e-5).all() and np.isfinite(z).all() and np.isfinite(nll).all()
    assert r[1] == -1.0 / 1e-5 and r[2] == 1.0 / 1e-5            # |y - p| = 1 - 4e-18 rounds to 1: no cancellation
    assert nll[3] == 0.0 and nll[4] == 0.0 and nll[1] == 40.0 + np.log1p(np.exp(-40.0))
    np.testing.assert_allclose(LG.prob(eta) + LG.prob(-eta), 1.0, rtol=0, atol=2.0 ** -52)


# ---- the residual's state after a step that rewrites r -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("glm_shim") / "_resid_glm_shim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                    os.path.join(HERE, "resid_glm_shim.cpp")], check=True)
    L = C.CDLL(so)
    vp, i64, f64, ci = C.c_void_p, C.c_int64, C.c_double, C.c_int
    x = [i64, vp, vp]
    for name, res, args in [("rg_new", vp, [i64]), ("rg_free", None, [vp]), ("rg_rebuild", ci, [vp] + x), ("rg_irls_apply", None, [vp]),
                            ("rg_rewritten", None, [vp]), ("rg_set_y", None, [vp]), ("rg_stream", None, [vp, i64]),
                            ("rg_moved", None, [vp, i64, f64]), ("rg_left_lazy", None, [vp] + x), ("rg_dots_taken", None, [vp, i64, ci]),
                            ("rg_consistent", ci, [vp]), ("rg_lazy", ci, [vp]), ("rg_owes", ci, [vp]), ("rg_roundings", i64, [vp]),
                            ("rg_skipped", i64, [vp]), ("rg_noop", ci, [vp] + x), ("rg_can_adopt", ci, [vp, ci, i64])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def _x(pairs):
    idx = np.array([k for k, _ in pairs], dtype=np.int64)
    val = np.array([v for _, v in pairs], dtype=np.float64)
    return len(pairs), idx.ctypes.data, val.ctypes.data, (idx, val)


def test_a_step_leaves_r_consistent_but_not_pristine(shim):
    L, p = shim, 9
    xa = _x([(2, 1.5), (5, -0.25)])
    s = L.rg_new(p)
    # initialize!(x), then the very same initialize! again: a no-op, skipped
    assert L.rg_rebuild(s, *xa[:3]) == 0 and L.rg_noop(s, *xa[:3]) == 1 and L.rg_rebuild(s, *xa[:3]) == 1
    assert L.rg_skipped(s) == 1
    L.rg_dots_taken(s, 2 * p, 1)
    assert L.rg_can_adopt(s, 1, p) == 1
    # the step: consistent with the iterate, but the buffer is d / w, not what initialize! writes; the stash is void
    L.rg_irls_apply(s)
    assert L.rg_consistent(s) == 1 and L.rg_owes(s) == 0 and L.rg_lazy(s) == 0 and L.rg_roundings(s) == 1
    assert L.rg_noop(s, *xa[:3]) == 0 and L.rg_can_adopt(s, 1, p) == 0
    assert L.rg_rebuild(s, *xa[:3]) == 0 and L.rg_skipped(s) == 1        # executed, not skipped
    assert L.rg_noop(s, *xa[:3]) == 1
    # whatever r owed before is void after a step (the export's catch-up has applied it): pending moves, a lazy residual
    L.rg_moved(s, 3, 0.5)
    assert L.rg_owes(s) == 1
    L.rg_rewritten(s)
    assert L.rg_owes(s) == 0 and L.rg_consistent(s) == 1
    L.rg_left_lazy(s, *xa[:3])
    assert L.rg_lazy(s) == 1
    L.rg_rewritten(s)
    assert L.rg_lazy(s) == 0 and L.rg_owes(s) == 0 and L.rg_consistent(s) == 1 and L.rg_noop(s, *xa[:3]) == 0
    # from an inconsistent residual too (a new y), and a streamed chunk afterwards counts its roundings from 1
    L.rg_set_y(s)
    assert L.rg_consistent(s) == 0
    L.rg_irls_apply(s)
    assert L.rg_consistent(s) == 1
    L.rg_stream(s, 3)
    assert L.rg_roundings(s) == 4 and L.rg_consistent(s) == 1
    L.rg_free(s)


# ---- the front end -----------------------------------------------------------------------------------------------------------
def test_refusals_that_precede_the_device():
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((12, 3)), (rng.random(12) < 0.5).astype(float)
    with pytest.raises(TypeError):
        cd.CDLogisticLoss(y, X.astype(np.float32))
    with pytest.raises(cd.DimensionMismatch):
        cd.CDLogisticLoss(y[:11], X)
    for cls in (cd.CDLeastSquaresLoss, cd.CDWeightedLSLoss, cd.CDQuadraticLoss):
        f = cls.__new__(cls)                  # (objects made without a device)
        with pytest.raises(TypeError):
            cd.logisticLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1))
        with pytest.raises(TypeError):
            cd.logisticLambdaMax(f)
        with pytest.raises(TypeError):
            cd.logisticLasso(f, None, 0.1)
    f = cd.CDLogisticLoss.__new__(cd.CDLogisticLoss)
    with pytest.raises(cd.ArgumentError, match="warmStart"):
        cd.logisticLasso_(cd.SparseIterate(3), f, cd.ProxL1(0.1), cd.CDOptions(warmStart=False))
    with pytest.raises(cd.ArgumentError, match="column of ones"):
        cd.logisticLasso(f, None, 0.1, fit_intercept=True)
    o = cd.IRLSOptions()
    assert (o.maxIter, o.optTol, o.wmin) == (25, 1e-7, 1e-5)


def test_new_symbols_are_declared_bound_and_cited():
    names = cd.declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    L = cd._lib.lib()
    for name, nargs in (("cdh_glm_set_labels", 3), ("cdh_glm_get_labels", 2), ("cdh_glm_irls", 4)):
        assert name in names and len(getattr(L, name).argtypes) == nargs, name
        before = hdr[: hdr.index("int32_t %s(" % name)]
        comment = before[before.rindex("/*"):]
        assert "no reference counterpart" in comment and "cd_differentiable_function.jl:118-194" in comment, name
        assert re.search(r"^int32_t %s\([^{;]*\) \{ return guarded\(h, \[&\]\(\) -> int32_t \{$" % name, src, flags=re.M), name
    jl = open(os.path.join(ROOT, "julia", "CoordinateDescentHIP.jl")).read()
    for name in ("cdh_glm_set_labels", "cdh_glm_get_labels", "cdh_glm_irls"):
        assert "(:%s, libcdhip)" % name in jl, name
    for n in ("CDLogisticLoss", "IRLSOptions", "logisticLasso_", "logisticLasso", "logisticLambdaMax", "LogisticLassoPath"):
        assert hasattr(cd, n), n
    assert issubclass(cd.CDLogisticLoss, cd.CDWeightedLSLoss)
    assert isinstance(cd.CDLogisticLoss.labels, property) and hasattr(cd.CDLogisticLoss, "irls_step")
    assert O.CDWeightedLSLoss is not None
