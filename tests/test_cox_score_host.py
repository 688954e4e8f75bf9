"""Score residuals, Schoenfeld residuals and the information matrix of the Cox lasso without a GPU: the twin's two halves
(tests/_cox_score_numpy.py) against each other; the column sums against the gradient of tests/_cox_strata_numpy.py; the
information matrix against central differences of that gradient, its symmetry and definiteness; the centring -- nothing moves
under a shift of a column with it, the matrix visibly does without it; an integer weight against replicated rows; coxInference's
numpy against the definition half; the front ends' refusals; the new prototype -- declared, bound, cited, guarded, in the Julia
binding and in INTEGRATION.md; where the kernels live and what they may not contain."""
import inspect
import os
import re

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_score_numpy as CSN
import _cox_strata_numpy as CS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")
LD = np.longdouble
U = 2.0 ** -53
KERNELS = ("k_score_centres", "k_score_centres_sum", "k_score_prep", "k_score_gather", "k_score_offsets", "k_score_scan", "k_score_mean", "k_score_rows",
           "k_score_info", "k_score_info_sum")


def _data(n, p, seed, strata=True, weights=True):
    """Times rounded to tenths (ties), three strata, weights, an offset, a dense beta of moderate size."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    time = np.round(rng.exponential(1.0, n), 1) + 0.1
    status = (rng.random(n) < 0.7).astype(np.float64)
    g = 3 * rng.integers(0, 3, n) - 1 if strata else None
    v = rng.uniform(0.25, 4.0, n) if weights else None
    off = rng.uniform(-0.3, 0.3, n)
    beta = rng.normal(0.0, 0.4, p)
    return dict(X=X, time=time, status=status, g=g, v=v, off=off, beta=beta)


def _call(fn, d, X=None, **kw):
    X = d["X"] if X is None else X
    return fn(X, d["X"] @ d["beta"], d["off"], d["time"], d["status"], 50.0, d["g"], d["v"], **kw)


@pytest.fixture(scope="module")
def sixty():
    d = _data(61, 4, 5)
    return d, _call(CSN.definition, d), _call(CSN.scan, d)


def test_the_two_halves_agree(sixty):
    d, a, b = sixty
    n = 61
    for k in ("sch", "score", "info"):
        scale = np.abs(b[k]).max()
        assert np.abs(a[k] - b[k]).max() <= 64 * n * 2.0 ** -64 * max(float(scale), 1.0), k
    assert np.array_equal(a["sch"][d["status"] == 0], np.zeros((int((d["status"] == 0).sum()), 4)))
    plain = _data(40, 3, 6, strata=False, weights=False)
    a, b = _call(CSN.definition, plain), _call(CSN.scan, plain)
    for k in ("sch", "score", "info"):
        assert np.abs(a[k] - b[k]).max() <= 64 * 40 * 2.0 ** -64 * max(float(np.abs(b[k]).max()), 1.0), k


def test_column_sums_are_the_gradient(sixty):
    """sum_i v_i L_ic and sum over the events of dv sch both equal X_c'(dv - ev A), the step twin's d."""
    d, a, b = sixty
    n = 61
    q = CS.rows(d["X"] @ d["beta"], d["off"], d["time"], d["status"], 1e-300, 50.0, exact=True, strata=d["g"], weights=d["v"])
    want = d["X"].T @ q["d"]
    size = np.abs(d["X"]).T @ (np.abs(q["delta"]) + np.abs(q["eA"]))
    for half in (a, b):
        got = (d["v"][:, None] * half["score"]).sum(axis=0).astype(np.float64)
        assert np.all(np.abs(got - want) <= 8 * n * U * size)
        got = ((d["v"] * d["status"])[:, None] * half["sch"]).sum(axis=0).astype(np.float64)
        assert np.all(np.abs(got - want) <= 8 * n * U * size)


def test_information_is_the_derivative_of_the_gradient(sixty):
    """Central differences of the twin's gradient n g(beta) = -X'(dv - ev A) in beta: error O(step^2) + O(U / step)."""
    d, a, _ = sixty
    n, p = d["X"].shape
    step = 1e-5
    H = np.zeros((p, p))
    for c in range(p):
        gs = []
        for sign in (+1.0, -1.0):
            b = d["beta"].copy()
            b[c] += sign * step
            gs.append(n * CS.gradient(d["X"], d["X"] @ b, d["off"], d["time"], d["status"], strata=d["g"], weights=d["v"])[0])
        H[:, c] = (gs[0] - gs[1]) / (2 * step)
    info = a["info"].astype(np.float64)
    assert np.abs(H - info).max() <= 1e-6 * np.abs(info).max()


def test_information_is_symmetric_and_positive_semidefinite(sixty):
    _, a, b = sixty
    for half in (a, b):
        info = half["info"].astype(np.float64)
        assert np.abs(info - info.T).max() <= 4 * U * np.abs(info).max()
        assert np.linalg.eigvalsh((info + info.T) / 2).min() >= -61 * U * np.abs(info).max()


def test_a_shift_of_a_column_changes_nothing_with_centring_and_the_matrix_without():
    """x_0 + 1e6.  With centring, every output is exactly invariant under a constant shift of xt, and the shifted xt differs from
    a constant shift by the rounding of the shifted entries and of their mean: |d xt_i0| <= 2 ulp(1e6) =: a per row, so xbar_0
    (a weighted mean) moves by at most a as well.  Then sch and every term xt_i - xbar_k of L move by at most 2 a:
    |d sch| <= 2 a, |d L| <= 2 a (1 + e A); and I, bilinear in xt, with T1_d = sum ev A |xt_d| and T2_d = sum dv Xabs_d:
    |d I_0d| <= 2 a max_d (T1_d + T2_d) + a^2 (sum ev A + sum dv).  (The halves' own long-double rounding is 2^-11 of this.)
    Without centring (centre 0) the two sums of I are each about 1e12 larger than I: it moves visibly."""
    d = _data(61, 3, 8)
    shifted = d["X"].copy()
    shifted[:, 0] += 1e6
    a = 2 * np.spacing(1e6)
    s = _call(CSN.scan, d)
    eA = (s["e"] * s["A"]).astype(np.float64)
    w, dk = (s["ev"] * s["A"]).astype(np.float64), np.where(s["counts"], s["dv"], 0).astype(np.float64)
    T = w @ np.abs(s["xt"]) + dk @ s["Xabs"].astype(np.float64)
    tol = 1.01 * (2 * a * T.max() + a * a * (w.sum() + dk.sum()))
    for fn in (CSN.definition, CSN.scan):
        q0, q1 = _call(fn, d), _call(fn, d, X=shifted)
        assert np.abs(q1["sch"] - q0["sch"]).max() <= 2 * a
        assert np.all(np.abs(q1["score"] - q0["score"]).astype(np.float64) <= 1.01 * 2 * a * (1 + eA[:, None]))
        assert np.abs(q1["info"] - q0["info"]).max() <= tol
        assert tol <= 1e-6 * np.abs(q0["info"]).max()              # (the bound itself is far below the matrix)
    zero = np.zeros(3)
    f0, f1 = _call(CSN.scan, d, centre=zero, dtype=np.float64), _call(CSN.scan, d, X=shifted, centre=zero, dtype=np.float64)
    assert np.abs(f1["info"][0, 0] - f0["info"][0, 0]) >= 1e-6 * abs(f0["info"][0, 0])


def test_an_integer_weight_is_a_replicated_row():
    """Breslow: weights 1, 2, 4 give the L and sch of the rows replicated that often (every copy the same) and the same I.
    (Powers of two: the float64 product v e that the kernels and the twin scan is then exact, and the two sides differ by the
    long-double summation order alone.)"""
    d = _data(40, 3, 9, weights=False)
    rng = np.random.default_rng(10)
    k = rng.choice([1, 2, 4], 40)
    rep = np.repeat(np.arange(40), k)
    eta = d["X"] @ d["beta"]
    centre = np.average(d["X"], axis=0, weights=k)
    w = CSN.definition(d["X"], eta, d["off"], d["time"], d["status"], 50.0, d["g"], k.astype(np.float64), centre=centre)
    r = CSN.definition(d["X"][rep], eta[rep], d["off"][rep], d["time"][rep], d["status"][rep], 50.0, d["g"][rep], None, centre=centre)
    for key in ("sch", "score"):
        assert np.abs(r[key] - w[key][rep]).max() <= 200 * 2.0 ** -64 * max(1.0, float(np.abs(w[key]).max()))
    assert np.abs(r["info"] - w["info"]).max() <= 200 * 2.0 ** -64 * float(np.abs(w["info"]).max())


def test_inference_against_the_definition_half():
    """n = 300, p = 8, three strata, weights: coxInferenceFrom on the scan half's answers against the definition half's."""
    d = _data(300, 8, 11)
    cluster = np.random.default_rng(12).integers(0, 40, 300)
    eta = d["X"] @ d["beta"]
    want = CSN.inference(d["X"], d["beta"], eta, d["off"], d["time"], d["status"], d["g"], d["v"], cluster)
    s = _call(CSN.scan, d)
    got = cd.coxInferenceFrom(np.arange(1, 9), d["beta"], s["info"].astype(np.float64), s["score"].astype(np.float64), d["v"], cluster)
    cond = np.linalg.cond(want["info"])
    for k in ("var", "se", "z", "dfbeta", "robust_var", "robust_se"):
        np.testing.assert_allclose(getattr(got, k), want[k], rtol=1e3 * U * cond, atol=0, err_msg=k)
    plain = cd.coxInferenceFrom(np.arange(1, 9), d["beta"], s["info"].astype(np.float64))
    assert plain.dfbeta is None and plain.robust_var is None and plain.robust_se is None
    np.testing.assert_array_equal(plain.se, got.se)
    each = cd.coxInferenceFrom(np.arange(1, 9), d["beta"], s["info"].astype(np.float64), s["score"].astype(np.float64), d["v"])
    np.testing.assert_allclose(each.robust_var, each.dfbeta.T @ each.dfbeta, rtol=1e-13)


def test_front_end_refusals():
    info = np.eye(2)
    with pytest.raises(cd.ArgumentError, match="singular"):
        cd.coxInferenceFrom([1, 2], [0.1, 0.2], np.ones((2, 2)))
    with pytest.raises(cd.DimensionMismatch):
        cd.coxInferenceFrom([1, 2], [0.1], info)
    with pytest.raises(cd.DimensionMismatch, match="cluster"):
        cd.coxInferenceFrom([1, 2], [0.1, 0.2], info, np.zeros((5, 2)), None, np.zeros(4))
    for fn in (cd.coxScoreResiduals, cd.coxSchoenfeldResiduals, cd.coxInformation, cd.coxInference):
        with pytest.raises(TypeError, match="takes a CDCoxLoss"):
            fn(object())
    f = cd.CDCoxLoss.__new__(cd.CDCoxLoss)
    f.n, f.p = 10, 70
    with pytest.raises(cd.ArgumentError, match="at most 64 columns"):
        f.score_residuals(np.arange(1, 66))
    with pytest.raises(cd.ArgumentError, match="outside 1 .. p"):
        f.information([0, 3])
    with pytest.raises(cd.ArgumentError, match="outside 1 .. p"):
        f.schoenfeld_residuals([71])
    with pytest.raises(cd.ArgumentError, match="non-empty vector"):
        f.information([])
    with pytest.raises(cd.ArgumentError, match="non-empty vector"):
        f.information([1.5])
    with pytest.raises(cd.ArgumentError, match="cluster needs robust=True"):
        cd.coxInference(f, [1], cluster=np.zeros(10))
    with pytest.raises(cd.DimensionMismatch, match="cluster"):
        cd.coxInference(f, [1], robust=True, cluster=np.zeros(9))
    with pytest.raises(cd.ArgumentError, match='type must be'):
        f.residuals("score")                                      # the three-type export keeps its three types


def test_api_names_and_defaults():
    for n in ("CoxSchoenfeld", "CoxInference", "coxScoreResiduals", "coxSchoenfeldResiduals", "coxInformation", "coxInference"):
        assert hasattr(cd, n), n
    sig = lambda fn: [(k, v.default) for k, v in inspect.signature(fn).parameters.items()][1:]
    assert sig(cd.CDCoxLoss.score_residuals) == [("columns", None), ("weighted", False), ("eta_max", 50.0)]
    assert sig(cd.CDCoxLoss.schoenfeld_residuals) == [("columns", None), ("eta_max", 50.0)]
    assert sig(cd.CDCoxLoss.information) == [("columns", None), ("eta_max", 50.0)]
    assert sig(cd.coxInference) == [("columns", None), ("robust", False), ("cluster", None), ("eta_max", 50.0)]
    assert list(cd.CoxSchoenfeld.__dataclass_fields__) == ["rows", "stratum", "time", "resid", "columns"]
    assert list(cd.CoxInference.__dataclass_fields__) == ["columns", "beta", "var", "se", "z", "dfbeta", "robust_var", "robust_se"]


def test_the_new_symbol_is_declared_bound_and_cited():
    name = "cdh_glm_cox_score"
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    assert name in cd.declared_symbols()
    before = hdr[: hdr.index("int32_t %s(" % name)]
    comment = " ".join(before[before.rindex("/*"):].replace(" * ", " ").split())
    for words in ("no reference counterpart", "cd_differentiable_function.jl:118-194", "1-based", "m > 64", "bit-identical run to run",
                  "is not offered with start-stop times yet", "is not offered with Efron ties yet", "all three outputs NULL",
                  "a handle put back to Breslow is served"):
        assert words in comment, words
    assert re.search(r"^int32_t %s\([^{;]*\) \{ return guarded\(h, \[&\]\(\) -> int32_t \{$" % name, src, flags=re.M)
    assert "(:%s, libcdhip)" % name in open(os.path.join(ROOT, "julia", "CoordinateDescentHIP.jl")).read()
    assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for words in ("score_residuals", "schoenfeld_residuals", "coxInference", "at most 64 columns"):
        assert words in readme, words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_score_gather" in design and "k_score_info" in design and "(32)" in design


def test_bound_and_a_null_handle_is_refused():
    L = cd._lib.lib()
    assert len(L.cdh_glm_cox_score.argtypes) == 9
    idx = np.ones(1, dtype=np.int64)
    out = np.zeros(4)
    assert L.cdh_glm_cox_score(None, 50.0, 1, idx.ctypes.data, None, None, out.ctypes.data, None, None) == cd._lib.CDH_BAD_ARG
    assert b"handle is NULL" in L.cdh_last_error(None)


def test_the_kernels_live_in_a_fifth_translation_unit():
    """cdhip.hip holds no score kernel: they are cox_score.hip's, the host body launches none, cox_efron_host.hpp stays the last
    include, the pad is what it was, and the build compiles the five files into the one library."""
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    unit = open(os.path.join(CSRC, "cox_score.hip")).read()
    host = open(os.path.join(CSRC, "cox_score_host.hpp")).read()
    assert src.rindex("#include") == src.index('#include "cox_efron_host.hpp"')
    assert src.index('#include "cox_concordance_host.hpp"') < src.index('#include "cox_score_host.hpp"') < src.index('extern "C" {')
    for k in KERNELS:
        assert re.search(r"void %s\(" % k, unit), k
        assert k not in re.sub(r"//[^\n]*", "", host) and k not in re.sub(r"//[^\n]*", "", src), k
    assert "hipLaunchKernelGGL" not in re.sub(r"//[^\n]*", "", host)
    code = re.sub(r"//[^\n]*", "", unit)
    assert code.count("#pragma clang fp contract(off)") >= 7
    assert not re.search(r"atomic|cooperative|__threadfence|while\s*\(\s*(?:true|1)\s*\)|volatile|asm", code)
    # the launches do not grow with m: no loop in the launch sequences
    tail = code[code.index("hipError_t cox_score_centres"):]
    assert not re.search(r"\b(for|while)\b", tail)
    iv = open(os.path.join(CSRC, "cox_interval.hpp")).read()
    assert "const unsigned char k_code_object_pad[0x10000 - 0x2a00] = {1};" in iv
    lib = open(os.path.join(ROOT, "coordinatedescent.jl_amd", "_lib.py")).read()
    for name in ("cdhip.hip", "cox_efron.hip", "cox_post.hip", "cox_concordance.hip", "cox_score.hip"):
        assert '"%s"' % name in lib, name
    plan = open(os.path.join(CSRC, "cox_plan.hpp")).read()
    assert "constexpr CoxScoreLayout cox_score_layout(int64_t ld, int64_t m)" in plan
    assert "cox_plan(h->ld, h->knobs.cox_grid)" in host and "getenv" not in host and "getenv" not in unit
