"""Harrell's concordance index of the Cox lasso without a GPU: the twin's two halves (tests/_cox_concordance_numpy.py) held
equal with ==; the new prototype -- declared, bound with the right arity, cited, guarded, in the Julia binding and in
INTEGRATION.md; the front ends' names and defaults; where the kernels live and what they may not contain."""
import inspect
import os
import re

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_concordance_numpy as CC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")

KERNELS = ("k_conc_tile", "k_conc_fringe", "k_conc_level", "k_conc_rows", "k_conc_total")
CASES = ("plain", "strata", "subset", "weights", "one time", "one eta", "no censoring")


def _sixty(case):
    """About 60 rows, times rounded to halves and eta to one decimal: ties in both."""
    rng = np.random.default_rng(40 + CASES.index(case))
    n = 61
    kw = dict(time=np.ceil(2.0 * rng.exponential(1.0, n)) / 2.0, status=(rng.random(n) < 0.65).astype(np.float64),
              eta=np.round(rng.normal(0.0, 0.6, n), 1))
    if case == "strata":
        kw["strata"] = 5 * rng.integers(0, 3, n) - 2
    if case == "subset":
        kw["subset"] = rng.random(n) < 0.6
    if case == "weights":
        kw.update(weights=rng.permutation(np.r_[np.full(30, 0.5), np.full(31, 1.5)]), strata=rng.integers(0, 2, n),
                  subset=rng.random(n) < 0.8)
    if case == "one time":
        kw["time"] = np.full(n, 2.5)
    if case == "one eta":
        kw["eta"] = np.where(rng.random(n) < 0.5, 0.0, -0.0)             # -0.0 == 0.0
    if case == "no censoring":
        kw["status"] = np.ones(n)
    return kw


# ---- the twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_the_two_halves_agree(case):
    kw = _sixty(case)
    a, b = CC.definition(**kw), CC.levels(**kw)
    assert a == b == CC.levels_vectorised(**kw), (a, b)
    c, d, t = a
    assert c + d + t > 0
    if case == "one eta":
        assert c == 0 and d == 0 and CC.cindex(c, d, t) == 0.5
    else:
        assert c > 0 and d > 0 and t > 0                              # the data do exercise all three
    if case == "one time":                                               # only (event, censored) pairs are comparable
        n_e, n_c = np.count_nonzero(kw["status"] == 1.0), np.count_nonzero(kw["status"] == 0.0)
        assert c + d + t == n_e * n_c
    if case == "no censoring":                                           # every pair of distinct times, once
        _, counts = np.unique(kw["time"], return_counts=True)
        assert c + d + t == (61 * 60 - np.sum(counts * (counts - 1))) // 2
    if case == "weights":
        assert any(float(x) != int(x) for x in a)                        # quarters do occur
        ld = CC.definition(**kw, dtype=np.longdouble)
        assert tuple(float(x) for x in ld) == a                          # quarters: exact in both


def test_a_hand_made_case():
    """Five rows: an event at t = 1, an event and a censored row at t = 2, two events at t = 3."""
    time, status = [1.0, 2.0, 2.0, 3.0, 3.0], [1.0, 1.0, 0.0, 1.0, 1.0]
    eta = [0.5, 0.5, 0.1, 0.9, -1.0]
    # row 0 against 1, 2, 3, 4: tied, concordant, discordant, concordant; row 1 against 2 (censored at its time), 3, 4:
    # concordant, discordant, concordant; rows 3 and 4: events at one time, not comparable
    assert CC.definition(time, status, eta) == (4.0, 2.0, 1.0) == CC.levels(time, status, eta)
    assert CC.cindex(4.0, 2.0, 1.0) == 4.5 / 7.0 and np.isnan(CC.cindex(0.0, 0.0, 0.0))


# ---- the prototype -------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_declared_bound_and_cited():
    name, nargs = "cdh_glm_cox_concordance", 3
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    L = cd._lib.lib()
    assert name in cd.declared_symbols() and len(getattr(L, name).argtypes) == nargs
    assert "int32_t cdh_glm_cox_concordance(cdh_handle h, int32_t k, double *out4);" in hdr
    before = hdr[: hdr.index("int32_t %s(" % name)]
    comment = before[before.rindex("/*"):]
    assert "no reference counterpart" in comment and "cd_differentiable_function.jl:118-194" in comment
    assert "concordance with start-stop times is not offered yet" in comment
    assert re.search(r"^int32_t %s\([^{;]*\) \{ return guarded\(h, \[&\]\(\) -> int32_t \{$" % name, src, flags=re.M)
    jl = open(os.path.join(ROOT, "julia", "CoordinateDescentHIP.jl")).read()
    assert re.search(r"ccall\(\(:%s, libcdhip\), Int32, \(Ptr\{Cvoid\}, Int32, Ptr\{Float64\}\)" % name, jl)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`%s`" % name in doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in KERNELS:
        assert k in design, k


def test_a_null_handle_is_refused():
    L = cd._lib.lib()
    out = np.zeros(4)
    assert L.cdh_glm_cox_concordance(None, -1, out.ctypes.data_as(cd._lib.C.POINTER(cd._lib.C.c_double))) == cd._lib.CDH_BAD_ARG
    assert b"handle is NULL" in L.cdh_last_error(None)


def test_the_kernels_live_in_a_fourth_translation_unit():
    """cdhip.hip and the host body hold no concordance kernel and launch none; the host body comes before cox_efron_host.hpp,
    which stays the last include; the pad is what it was; the build compiles the four files into the one library."""
    src = open(os.path.join(CSRC, "cdhip.hip")).read()
    unit = open(os.path.join(CSRC, "cox_concordance.hip")).read()
    host = open(os.path.join(CSRC, "cox_concordance_host.hpp")).read()
    shared = open(os.path.join(CSRC, "cox_concordance.hpp")).read()
    assert src.rindex("#include") == src.index('#include "cox_efron_host.hpp"')
    assert src.index('#include "cox_post_host.hpp"') < src.index('#include "cox_concordance_host.hpp"') < src.index('extern "C" {')
    for k in KERNELS:
        assert re.search(r"void %s\(" % k, unit), k
        for text in (host, src, shared):
            assert k not in re.sub(r"//[^\n]*", "", text), k
    assert "hipLaunchKernelGGL" not in re.sub(r"//[^\n]*", "", host) and "__global__" not in host and "__global__" not in shared
    code = re.sub(r"//[^\n]*", "", unit)
    assert code.count("#pragma clang fp contract(off)") == len(KERNELS)
    assert not re.search(r"atomic|cooperative|__threadfence|while\s*\(\s*(?:true|1)\s*\)|volatile|asm|getenv", code)
    assert "getenv" not in host and "block_sum<" in code
    iv = open(os.path.join(CSRC, "cox_interval.hpp")).read()
    assert "const unsigned char k_code_object_pad[0x10000 - 0x2a00] = {1};" in iv
    lib = open(os.path.join(ROOT, "coordinatedescent.jl_amd", "_lib.py")).read()
    for f in ("cdhip.hip", "cox_efron.hip", "cox_post.hip", "cox_concordance.hip"):
        assert 'os.path.join(CSRC, "%s")' % f in lib, f
    assert "cox_concordance.hip" in cd._lib._sources() and "cox_concordance_host.hpp" in cd._lib._sources()
    plan = open(os.path.join(CSRC, "cox_plan.hpp")).read()
    assert "constexpr CoxConcLayout cox_conc_layout(int64_t ld)" in plan and "constexpr CoxConcTake cox_conc_take(" in plan
    assert "cox_conc_take(" in code and "cox_conc_fringe(" in code       # the kernels share the tests' arithmetic


# ---- the front ends ------------------------------------------------------------------------------------------------------------
def test_api_names_and_defaults():
    for n in ("CoxConcordance", "coxConcordance", "CVCoxConcordancePathResult"):
        assert hasattr(cd, n), n
    p = inspect.signature(cd.CDCoxLoss.concordance).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("fold", None)]
    assert [(k, v.default) for k, v in inspect.signature(cd.coxConcordance).parameters.items()] == [("f", inspect.Parameter.empty), ("fold", None)]
    assert list(cd.CoxConcordance.__dataclass_fields__) == ["concordant", "discordant", "tied", "comparable", "C"]
    assert issubclass(cd.CVCoxConcordancePathResult, cd.CVCoxLassoPathResult)
    base = list(cd.CVCoxLassoPathResult.__dataclass_fields__)
    assert "fold_concordance" not in base
    assert list(cd.CVCoxConcordancePathResult.__dataclass_fields__) == base + ["fold_concordance"]
    assert inspect.signature(cd.cvCoxLassoPath).parameters["measure"].default == "deviance"
    for fn, words in ((cd.CDCoxLoss.concordance, ("survival::concordance", "Cindex")), (cd.coxConcordance, ("survival::concordance",)),
                      (cd.cvCoxLassoPath, ('measure="C"', "LARGEST"))):
        for w in words:
            assert w in fn.__doc__, (fn, w)
    with pytest.raises(TypeError):
        cd.coxConcordance(object())
    f = cd.CDCoxLoss.__new__(cd.CDCoxLoss)
    with pytest.raises(cd.ArgumentError, match="fold must be"):
        f.concordance(fold=-2)
    X, y = np.zeros((4, 2)), np.array([[1.0, 1.0], [2.0, 0.0], [3.0, 1.0], [4.0, 0.0]])
    for bad in ("class", "c", None):
        with pytest.raises(cd.ArgumentError, match="measure"):
            cd.cvCoxLassoPath(X, y, [0.1], K=2, measure=bad)
