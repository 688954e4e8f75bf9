"""Residuals, the baseline hazard and survival curves of the Cox lasso without a GPU: the twin's two halves
(tests/_cox_post_numpy.py) against each other for the four chains, and against the sibling twins' A; the martingale residuals'
sum per stratum; coxSurvival on hand-made tables; the two new prototypes -- declared, bound with the right arity, cited, guarded,
in the Julia binding and in INTEGRATION.md; where the kernels live and what they may not contain."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_efron_numpy as CE
import _cox_interval_numpy as CI
import _cox_post_numpy as CPN
import _cox_strata_numpy as CS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")
LD = np.longdouble

NEW_SYMBOLS = (("cdh_glm_cox_residuals", 5), ("cdh_glm_cox_baseline", 10))
KERNELS = ("k_post_rows", "k_post_mark", "k_post_offsets", "k_post_scan", "k_post_flag", "k_post_scatter")
CHAINS = ("plain", "strata", "interval", "efron")


def _sixty(chain):
    """About 60 rows with times rounded to halves (heavy ties); strata and weights unless the chain is plain; an offset."""
    rng = np.random.default_rng(21 + CHAINS.index(chain))
    n = 61
    stop = np.ceil(2.0 * rng.exponential(1.0, n)) / 2.0 + 0.5
    status = (rng.random(n) < 0.7).astype(np.float64)
    g = None if chain == "plain" else 5 * rng.integers(0, 3, n) - 2
    v = None if chain == "plain" else rng.uniform(0.25, 4.0, n)
    start = None
    if chain == "interval":
        start = np.floor(2.0 * stop * rng.uniform(0.0, 0.9, n)) / 2.0      # halves: starts coincide with event times
        assert np.all(start < stop)
    eta = rng.normal(0.0, 0.7, n)
    off = rng.uniform(-0.5, 0.5, n)
    return dict(eta_lin=eta, off=off, stop=stop, status=status, eta_max=float(np.quantile(eta + off, 0.9)), strata=g, weights=v, start=start,
                ties="efron" if chain == "efron" else "breslow")


# ---- the twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_the_two_halves_agree(chain):
    kw = _sixty(chain)
    a, b = CPN.definition(**kw), CPN.scan(**kw)
    n = len(kw["stop"])
    # the scan half takes S from the sibling twins' exact forms, which round it to float64 once (the Efron twin is long double
    # throughout); the subtraction in S (start-stop) or den (Efron) magnifies that by rho
    tol = 8 * 2.0 ** -53 * b["rho"]
    assert n == len(b["rho"]) and np.any(kw["eta_lin"] + kw["off"] > kw["eta_max"])     # some rows cap
    assert np.all(np.abs(a["cumhaz"] - b["cumhaz"]) <= tol * b["Asz"])
    assert np.all(np.abs(a["martingale"] - b["martingale"]) <= tol * b["e"] * b["Asz"])
    # the deviance residual through its square: the subtraction in M + log(eA) cancels near eA = 1
    d2a, d2b = a["deviance"] ** 2, b["dev2"]
    assert np.all(np.abs(d2a - d2b) <= 4 * tol * (np.abs(b["martingale"]) + np.abs(b["lg"]) + b["e"] * b["Asz"] + b["delta"]))
    assert np.array_equal(np.sign(a["deviance"]), np.sign(b["deviance"]))
    ta, tb = a["table"], b["table"]
    assert np.array_equal(ta["stratum"], tb["stratum"]) and np.array_equal(ta["time"], tb["time"])
    assert len(ta["time"]) >= 8 and np.any(np.diff(ta["stratum"]) != 0) == (chain != "plain")
    for key in CPN.COLUMNS[2:]:
        size = tb["Ssz"] if key == "risk_sum" else np.abs(tb[key])
        assert np.all(np.abs(ta[key] - tb[key]) <= 16 * 2.0 ** -53 * tb["rho"] * size), key
    if chain == "efron":                                         # the data do exercise l >= 2, and Efron is not Breslow here
        assert np.max(tb["n_event"] / kw["weights"].min()) >= 3
        c = CPN.scan(**dict(kw, ties="breslow"))
        assert np.max(np.abs(c["cumhaz"] - b["cumhaz"])) > 1e-3


@pytest.mark.parametrize("chain", CHAINS)
def test_the_scan_half_reads_the_sibling_twins_A(chain):
    """cumhaz is the A of the step's twins: the exact forms of _cox_strata_numpy and _cox_interval_numpy, _cox_efron_numpy in long
    double."""
    kw = _sixty(chain)
    b = CPN.scan(**kw)
    args = (kw["eta_lin"], kw["off"], kw["stop"], kw["status"], 1e-300, kw["eta_max"])
    sw = dict(strata=kw["strata"], weights=kw["weights"])
    if chain == "efron":
        want, tol = CE.rows(*args, dtype=LD, **sw)["A"], 2.0 ** -52 * np.abs(b["cumhaz"])
    elif chain == "interval":
        want = CI.rows(args[0], args[1], kw["start"], *args[2:], exact=True, **sw)["A"]
        tol = 8 * 2.0 ** -53 * b["Asz"]
    else:
        want, tol = CS.rows(*args, exact=True, **sw)["A"], 8 * 2.0 ** -53 * np.abs(b["cumhaz"])
    assert np.all(np.abs(b["cumhaz"] - want) <= tol)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("half", ("definition", "scan"))
def test_weighted_martingale_residuals_sum_to_zero_per_stratum(chain, half):
    """sum of v_i M_i over a stratum = sum dv - sum over the event groups of (their increment's total share) = 0: the score
    equation of an intercept, for Breslow and for Efron, with and without start times."""
    kw = _sixty(chain)
    q = getattr(CPN, half)(**kw)
    n = len(kw["stop"])
    v = np.ones(n) if kw["weights"] is None else kw["weights"]
    g = np.zeros(n, dtype=int) if kw["strata"] is None else kw["strata"]
    for s in np.unique(g):
        m = g == s
        total = CPN._lsum(v[m] * q["martingale"][m])
        scale = CPN._lsum(v[m] * (kw["status"][m] + np.abs(kw["status"][m] - q["martingale"][m])))
        assert abs(total) <= 64 * n * 2.0 ** -64 * scale, (chain, s, total)


# ---- coxSurvival -----------------------------------------------------------------------------------------------------------------
def _table(stratum, time, cumhaz):
    z = np.zeros(len(time))
    return cd.CoxBaseline(np.asarray(stratum, dtype=np.int32), np.asarray(time, dtype=np.float64), z, z, z,
                          np.asarray(cumhaz, dtype=np.float64), z)


def test_survival_curves_on_hand_made_tables():
    one = _table([0, 0, 0], [1.0, 2.0, 4.0], [0.25, 0.5, 1.5])
    eta = np.array([0.0, math.log(2.0)])
    times = [0.5, 1.0, 1.5, 2.0, 4.0, 100.0]                    # before the first event, at event times, between, beyond the last
    S = cd.coxSurvival(one, eta, times)
    H = np.array([0.0, 0.25, 0.25, 0.5, 1.5, 1.5])
    np.testing.assert_array_equal(S, np.exp(-H[None, :] * np.exp(eta)[:, None]))
    np.testing.assert_array_equal(S[:, 0], 1.0)                  # nothing has happened yet
    assert S.shape == (2, 6) and np.all(np.diff(S, axis=1) <= 0.0) and np.all((S > 0.0) & (S <= 1.0))
    np.testing.assert_allclose(S, CPN.survival(dict(stratum=one.stratum, time=one.time, cumhaz=one.cumhaz), eta, times, [0, 0]),
                               rtol=4e-16)
    # two strata, with ids that are not consecutive; a new row reads its own stratum's step function
    two = _table([-3, -3, 7], [1.0, 3.0, 2.0], [0.1, 0.4, 0.9])
    S2 = cd.coxSurvival(two, [0.0, 0.0, 0.5], [0.5, 1.0, 2.0, 3.0], strata_new=[-3, 7, 7])
    np.testing.assert_array_equal(S2[0], np.exp(-np.array([0.0, 0.1, 0.1, 0.4])))
    np.testing.assert_array_equal(S2[1], np.exp(-np.array([0.0, 0.0, 0.9, 0.9])))
    np.testing.assert_array_equal(S2[2], np.exp(-np.array([0.0, 0.0, 0.9, 0.9]) * np.exp(0.5)))
    np.testing.assert_allclose(S2, CPN.survival(dict(stratum=two.stratum, time=two.time, cumhaz=two.cumhaz), [0.0, 0.0, 0.5],
                                                [0.5, 1.0, 2.0, 3.0], [-3, 7, 7]), rtol=4e-16)
    assert cd.coxSurvival(one, 0.0, 2.0).shape == (1, 1)         # scalars are a 1 x 1 problem


def test_survival_refusals():
    two = _table([-3, -3, 7], [1.0, 3.0, 2.0], [0.1, 0.4, 0.9])
    with pytest.raises(cd.ArgumentError, match="stratum 5 is not in the baseline table"):
        cd.coxSurvival(two, [0.0, 0.0], [1.0], strata_new=[7, 5])
    with pytest.raises(cd.ArgumentError, match="strata_new must name"):
        cd.coxSurvival(two, [0.0], [1.0])
    with pytest.raises(cd.DimensionMismatch):
        cd.coxSurvival(two, [0.0, 0.0], [1.0], strata_new=[7])


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
    jl = open(os.path.join(ROOT, "julia", "CoordinateDescentHIP.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in NEW_SYMBOLS:
        assert "(:%s, libcdhip)" % name in jl, name
        assert "`%s`" % name in doc, name
    for text in (hdr, open(os.path.join(ROOT, "README.md")).read(), doc):
        assert "Efron ties are offered for right-censored data; not yet with start" in " ".join(text.replace(" * ", " ").split())
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_post_rows" in design and "k_post_scatter" in design


def test_a_null_handle_is_refused():
    L = cd._lib.lib()
    BAD = cd._lib.CDH_BAD_ARG
    out = np.zeros(4)
    cnt = np.zeros(1, dtype=np.int64)
    p = out.ctypes.data
    assert L.cdh_glm_cox_residuals(None, 50.0, p, p, p) == BAD
    assert b"handle is NULL" in L.cdh_last_error(None)
    assert L.cdh_glm_cox_baseline(None, 50.0, 4, None, p, p, p, p, p, cnt.ctypes.data_as(cd._lib.C.POINTER(cd._lib.C.c_int64))) == BAD
    assert b"handle is NULL" in L.cdh_last_error(None)


def test_the_kernels_live_in_a_third_translation_unit():
    """cdhip.hip holds no post kernel: they are cox_post.hip's, the host body launches none, cox_efron_host.hpp stays the last
    include, the pad is what it was, and the build compiles the three files into the one library."""
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    unit = open(os.path.join(CSRC, "cox_post.hip")).read()
    host = open(os.path.join(CSRC, "cox_post_host.hpp")).read()
    assert src.rindex("#include") == src.index('#include "cox_efron_host.hpp"')
    assert src.index('#include "cox_kernels.hpp"') < src.index('#include "cox_post_host.hpp"') < src.index('extern "C" {')
    for k in KERNELS:
        assert re.search(r"void %s\(" % k, unit), k
        assert k not in re.sub(r"//[^\n]*", "", host) and k not in re.sub(r"//[^\n]*", "", src), k
    assert "hipLaunchKernelGGL" not in re.sub(r"//[^\n]*", "", host)
    code = re.sub(r"//[^\n]*", "", unit)
    assert "#pragma clang fp contract(off)" in code
    assert not re.search(r"atomic|cooperative|__threadfence|while\s*\(\s*(?:true|1)\s*\)|volatile|asm", code)
    iv = open(os.path.join(CSRC, "cox_interval.hpp")).read()
    assert "const unsigned char k_code_object_pad[0x10000 - 0x2a00] = {1};" in iv
    lib = open(os.path.join(ROOT, "coordinatedescent.jl_amd", "_lib.py")).read()
    assert '"cdhip.hip"' in lib and '"cox_efron.hip"' in lib and '"cox_post.hip"' in lib
    plan = open(os.path.join(CSRC, "cox_plan.hpp")).read()
    assert "constexpr CoxPostLayout cox_post_layout(int64_t ld)" in plan
    assert "cox_plan(h->ld, h->knobs.cox_grid)" in host and "getenv" not in host and "getenv" not in unit


# ---- the front ends ------------------------------------------------------------------------------------------------------------
def test_api_names_and_defaults():
    for n in ("CoxBaseline", "coxResiduals", "coxBaselineHazard", "coxSurvival"):
        assert hasattr(cd, n), n
    p = inspect.signature(cd.CDCoxLoss.residuals).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("type", "martingale"), ("eta_max", 50.0)]
    p = inspect.signature(cd.CDCoxLoss.baseline_hazard).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("eta_max", 50.0)]
    assert list(cd.CoxBaseline.__dataclass_fields__) == ["stratum", "time", "n_event", "risk_sum", "hazard", "cumhaz", "cumvar"]
    assert list(inspect.signature(cd.coxSurvival).parameters) == ["baseline", "eta_new", "times", "strata_new"]
    assert inspect.signature(cd.coxResiduals).parameters["type"].default == "martingale"
    for fn, words in ((cd.CDCoxLoss.residuals, ("residuals(coxph", "uncentred")), (cd.CDCoxLoss.baseline_hazard, ("basehaz", "uncentred")),
                      (cd.coxSurvival, ("survfit", "uncentred")), (cd.coxBaselineHazard, ("basehaz", "uncentred"))):
        for w in words:
            assert w in fn.__doc__, (fn, w)
    f = cd.CDCoxLoss.__new__(cd.CDCoxLoss)
    with pytest.raises(cd.ArgumentError, match="type must be"):
        f.residuals("score")
    with pytest.raises(TypeError):
        cd.coxResiduals(object())
    with pytest.raises(TypeError):
        cd.coxBaselineHazard(object())
