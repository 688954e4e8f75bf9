"""The GLM steps and solves on the device where weights clamp and exp saturates: the three families of k_glm_step
(csrc/glm_kernels.hpp) on the tables of tests/_glm_extremes.py -- |eta| up to 800, subnormal and vanished exp, rows on either
side of the clamp and of the cap, counts of 0 and 1e300, a deviance of +inf -- and the front ends on linearly separable labels
and on exposures sixteen powers of e apart, on the three kinds of handle.  The reference is the numpy twin of each family
(tests/_logistic_numpy.py, tests/_poisson_numpy.py), whose exp tests/test_glm_extremes_host.py holds to mpmath on every
argument that occurs here; on top of it stand the facts that hold exactly whatever the library's exp returns.

eta is injected, not fitted (tests/_glm_extremes.py), and every case asserts that the kernel's eta = y - r is the table's value
bit for bit before it steps.  wmin = 2^-17: on a clamped row r = d / wmin is exact, so where d is e or -mu the device's own
exp is read back from r.  A row's nll and deviance leave the kernels only in sums: they are read row by row as the held-out sum
of a fold that holds that one row (read-only, before the step that rewrites y and r).

Every case prints the figure it asserts on; LAB_NOTES.md "GLM extremes" holds the ones measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cv_logistic_numpy as CL
import _glm_extremes as GX
import _glm_plan as GP
import _logistic_numpy as LG
import _poisson_numpy as PN

pytestmark = pytest.mark.gpu

U, TINY, WMIN = GX.U, GX.TINY, GX.WMIN
NORMAL_MIN = 2.0 ** -1022
# The device's exp against numpy's, in spacings of the result (2^-1074 in the subnormal range), measured on an MI355X over both
# tables (test_device_exp_read_back); the bound is max(measured, 1) + 2: one spacing is numpy's own error
# (tests/test_glm_extremes_host.py), one is margin.
EXP_MEASURED = {"normal": 1.0, "subnormal": 0.0}
EXP_BOUND = {k: max(v, 1.0) + 2.0 for k, v in EXP_MEASURED.items()}


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _po(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _irls(f, apply, wmin=WMIN):
    out = np.zeros(3)
    cd.check(f._L.cdh_glm_irls(f._h, int(apply), float(wmin), _po(out)), f._h)
    return out


def _fold(f, k, apply, wmin=WMIN):
    out = np.zeros(5)
    cd.check(f._L.cdh_glm_irls_fold(f._h, int(k), int(apply), float(wmin), _po(out)), f._h)
    return out


def _pstep(f, k, apply, eta_max, wmin=WMIN):
    out = np.zeros(6)
    cd.check(f._L.cdh_glm_poisson_irls(f._h, int(k), int(apply), float(wmin), float(eta_max), _po(out)), f._h)
    return out


def _wmoments(f):
    sw, swr2 = C.c_double(), C.c_double()
    cd.check(f._L.cdh_resid_wmoments(f._h, C.byref(sw), C.byref(swr2)), f._h)
    return sw.value, swr2.value


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _inject(monkeypatch, cap, make, eta_lin, seed):
    """A handle whose stored y - r is eta_lin bit for bit: column 1 of X is eta_lin and the iterate (1.0, 0)."""
    if cap != GP.MAX_GRID:
        monkeypatch.setenv("CDH_GLM_GRID", str(cap))          # read when the handle is made
    f = make(GX.design(eta_lin, seed))
    x = cd.SparseIterate(2)
    x[1] = 1.0
    cd.initialize_(f, x)
    assert np.array_equal(f.y - f.r, eta_lin) and np.array_equal(f.y, np.zeros(len(eta_lin)))
    return f


def _one_row(f, i, step):
    """The held-out sums of a fold that holds row i alone, read-only: the row's own nll (deviance) and miss, exactly -- a
    sum of one term and zeros."""
    ids = np.zeros(f.n, dtype=np.int32)
    ids[i] = 1
    f.set_folds(ids, 2)
    return step(f, 1, 0)


def _first_rows(e):
    """The first row of every table entry that occurs in e."""
    return np.unique(e, return_index=True)[1]


def _spacings(dev, ref):
    """|dev - ref| in spacings of ref (2^-1074 where ref is subnormal or zero) -> (distances, normal-range mask)."""
    normal = ref >= NORMAL_MIN
    sp = np.where(normal, np.spacing(np.where(normal, ref, 1.0)), TINY)
    return np.abs(dev - ref) / sp, normal


def _worst(d, normal):
    return {"normal": float(d[normal].max()) if normal.any() else 0.0, "subnormal": float(d[~normal].max()) if (~normal).any() else 0.0}


def _exp_ok(d, normal):
    return bool(np.all(d[normal] <= EXP_BOUND["normal"]) and np.all(d[~normal] <= EXP_BOUND["subnormal"]))


# ---- a. the binomial step on its table ---------------------------------------------------------------------------------------------
def _binomial(monkeypatch, case):
    n, cap, branch, start = case
    GX.reaches(n, cap, branch)
    e = GX.entries(len(GX.B_TABLE[0]), n, start)
    eta, lab = GX.B_TABLE[0][e], GX.B_TABLE[1][e]
    return e, eta, lab, (lambda: _inject(monkeypatch, cap, lambda X: cd.CDLogisticLoss(lab, X), eta, n + start))


def _binomial_masks(eta, lab):
    """one: 1 + exp(-|eta|) rounds to 1 (|eta| >= 37.5 in the table; the device's e is far too close to numpy's to differ
    here).  There a hard label classified wrongly has d = -+1 and nll = |eta|, one classified rightly d = +-e."""
    one = (1.0 + np.exp(-np.abs(eta))) == 1.0
    hard = (lab == 0.0) | (lab == 1.0)
    right = one & hard & ((lab == 1.0) == (eta > 0.0))
    return one, right, one & hard & ~right


def _binomial_e(eta, r, right):
    """The device's exp(-|eta|) on the rightly classified rows, read back from r = +-e / wmin, with numpy's."""
    return np.abs(r[right]) * WMIN, np.exp(-np.abs(eta[right]))


@pytest.mark.parametrize("case", GX.B_CASES, ids=GX.case_id)
def test_binomial_step_on_the_table(monkeypatch, case):
    """Both APPLY forms.  Against the twin: w and r at 64 2^-53 relative, z at 64 2^-53 (|eta| + |r|), a row's nll at
    64 2^-53 of the operands of its subtraction; where r is +-e / wmin with e subnormal, e by test_device_exp_read_back's
    bound in spacings instead.  Exactly, whatever exp returns: (w == wmin) is the twin's flag row by row, z == eta + r, a hard
    label classified wrongly beyond |eta| = 37.5 has r == -+1 / wmin and nll == |eta|, one classified rightly has
    r == +-e / wmin, not bit-zero up to 745.13 and zero at 800, and nll == that e (eta < 0; glm_row takes e for log1p(e)
    where 1 + e == 1, see test_nll_of_a_rightly_classified_row_is_the_device_e) or 0 (eta > 0); nothing is NaN or infinite; the read-only sums are the applied ones bit for bit; the pad rows are zero through the weighted moments.
    Measured on an MI355X: 0.00 ulp on w, r, z and nll in all six cases -- every row the twin's bits, but for the e at
    |eta| = 708, one spacing (2^-1074 there) off; LAB_NOTES "GLM extremes"."""
    e, eta, lab, make = _binomial(monkeypatch, case)
    n = len(eta)
    f = make()
    w_t, z_t, r_t, nll_t, cl_t = LG.rows(lab, eta, WMIN)
    one, right, wrong = _binomial_masks(eta, lab)
    rows = _first_rows(e)
    nll = {int(i): _one_row(f, i, _fold) for i in rows}                         # read-only, before y and r are rewritten
    ro = _irls(f, 0)
    out = _irls(f, 1)
    assert np.array_equal(ro, out)
    w, z, r = f.w, f.y, f.r
    assert np.isfinite(np.r_[w, z, r, out]).all()
    # exactly
    assert np.array_equal(w == WMIN, cl_t) and (w[np.abs(eta) >= 40.0] == WMIN).all() and out[2] == cl_t.sum()
    assert np.array_equal(z, eta + r)
    assert np.array_equal(r[wrong], -np.sign(eta[wrong]) / WMIN) and wrong.sum() >= 3
    e_dev, e_np = _binomial_e(eta, r, right)
    assert (np.sign(r[right]) * np.sign(eta[right]) >= 0.0).all() and right.sum() >= 3
    assert (e_dev[np.abs(eta[right]) <= 745.13] > 0.0).all() and (e_dev[np.abs(eta[right]) >= 800.0] == 0.0).all()
    d, normal = _spacings(e_dev, e_np)
    # against the twin
    slack = np.where(right, EXP_BOUND["subnormal"] * TINY / WMIN, 0.0)            # (r of a subnormal e: spacings, not ulps)
    ew = np.abs(w - w_t) / w_t
    er = (np.abs(r - r_t) - slack) / np.where(r_t != 0.0, np.abs(r_t), 1.0)
    ez = (np.abs(z - z_t) - slack) / np.maximum(np.abs(eta) + np.abs(r_t), TINY)
    worst_nll = 0.0
    for i, o5 in nll.items():
        assert o5[4] == CL.miss(lab[i], eta[i]) and np.isfinite(o5).all()
        if wrong[i]:
            assert o5[3] == abs(eta[i]), (i, eta[i], o5)
        elif right[i]:
            assert o5[3] == (np.abs(r[i]) * WMIN if eta[i] < 0.0 else 0.0), (i, eta[i], o5, r[i])
        else:
            scale = max(eta[i], 0.0) + np.log1p(np.exp(-abs(eta[i]))) + abs(lab[i] * eta[i])
            worst_nll = max(worst_nll, abs(o5[3] - nll_t[i]) / scale)
    print(f"binomial extremes {GX.case_id(case)}: worst ulps w {ew.max() / U:.2f} r {er.max() / U:.2f} z {ez.max() / U:.2f} "
          f"nll {worst_nll / U:.2f}; exp read back on {right.sum()} rows, worst spacings {_worst(d, normal)}; clamped {int(out[2])}")
    assert np.all(ew <= 64 * U) and np.all(er <= 64 * U) and np.all(ez <= 64 * U) and worst_nll <= 64 * U
    assert _exp_ok(d, normal)
    assert abs(out[1] - w_t.sum()) <= (n + 64) * U * w_t.sum()
    assert abs(out[0] - nll_t.sum()) <= (n + 64) * U * np.abs(nll_t).sum()
    sw, swr2 = _wmoments(f)
    assert abs(sw - w.sum()) <= n * U * w.sum() and abs(swr2 - (w * r * r).sum()) <= 2 * n * U * (w * r * r).sum()
    f.close()


def test_nll_of_a_rightly_classified_row_is_the_device_e(monkeypatch):
    """Beyond |eta| = 37.5 a label-0 row at eta < 0 has nll = (0 + log1p(e)) - 0 with e < 2^-53, and log1p(e) = e - e^2 / 2 + ...
    rounds to e: nll == the device's own e, bit for bit, on every such row of the table (and == 0 at label 1, eta > 0).

    This test found a flaw, since mended in glm_row.  With nll = (max(eta, 0) + log1p(e)) - y eta as first written, 5 of the 11
    rows at eta < 0 were one spacing (2^-1074) off e on an MI355X -- at eta = -708.4 (e = 2.217119081664265e-308 against nll
    ...647e-308), -740 (e = 4.2e-322) and -744.44, -745 and -745.13 (e = 2^-1074, nll = 0: bit-zero before 746) --, every one
    with a subnormal e whose last bit is odd.  The cause was the device library's log1p: it takes no shortcut for small
    arguments but forms (a - 1) / (a + 1) for a = 1 + e held as the pair (1, e), as fl(e * rcp(2)) plus a remainder term;
    halving a subnormal e with an odd last bit is inexact, the remainder (half a spacing) underflows to zero, and the final
    ldexp(., 1) returns e with its last bit rounded to even.  glm_row now takes e itself where 1 + e == 1, which is log1p(e)
    correctly rounded there; every other row keeps the library's value, and the twin is unchanged."""
    case = [c for c in GX.B_CASES if c[0] == GP.ROWS + 1][0]
    e, eta, lab, make = _binomial(monkeypatch, case)
    f = make()
    _, right, _ = _binomial_masks(eta, lab)
    rows = [int(i) for i in _first_rows(e) if right[i]]
    nll = np.array([_one_row(f, i, _fold)[3] for i in rows])
    _irls(f, 1)
    r = f.r[rows]
    f.close()
    want = np.where(eta[rows] < 0.0, np.abs(r) * WMIN, 0.0)
    off = np.abs(nll - want) / TINY
    print(f"nll against the device's e on {len(rows)} rightly classified rows: {int((off > 0).sum())} differ, by at most {off.max():.0f} "
          f"spacings, at eta {eta[rows][off > 0].tolist()} (e {want[off > 0].tolist()})")
    assert len(rows) == 2 * 11                              # the table's |eta| from 37.5 to 800, either sign
    assert np.array_equal(nll, want)


# ---- b. the fold step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GX.B_CASES, ids=GX.case_id)
def test_binomial_fold_step_on_the_table(monkeypatch, case):
    """A third of the rows held out, saturated rows on both sides (tests/test_glm_extremes_host.py).  Held-out rows: w == 0 --
    never wmin --, r == 0 and z the bits of eta; held_miss exact, the eta = 0 row counted as class 0; held_nll within the
    summation bound; the training rows the plain step's rows bit for bit.  With k = -1 the vectors and the first three sums
    are the plain step's, bit for bit.  Measured on an MI355X: held nll 0.00 ulp of its sum in five cases, 1.42 in one."""
    e, eta, lab, make = _binomial(monkeypatch, case)
    n = len(eta)
    held = GX.third(n)
    tr = ~held
    fa, fb, fc = make(), make(), make()
    fa.set_folds(np.where(held, 1, 2 * (np.arange(n) % 2)).astype(np.int32), 3)
    w_t, z_t, r_t, nll_t, cl_t = LG.rows(lab, eta, WMIN)
    plain_ro = _irls(fb, 0)
    none_ro = _fold(fa, -1, 0)
    assert np.array_equal(none_ro[:3], plain_ro) and none_ro[3] == 0.0 and none_ro[4] == 0.0
    ro = _fold(fa, 1, 0)
    out = _fold(fa, 1, 1)
    plain, none = _irls(fb, 1), _fold(fc, -1, 1)
    assert np.array_equal(ro, out) and np.array_equal(plain, plain_ro) and np.isfinite(out).all()
    assert np.array_equal(none[:3], plain) and none[3] == 0.0 and none[4] == 0.0
    for u, v in ((fc.w, fb.w), (fc.y, fb.y), (fc.r, fb.r)):
        assert np.array_equal(_bits(u), _bits(v))
    w, z, r = fa.w, fa.y, fa.r
    assert np.array_equal(w[held], np.zeros(held.sum())) and np.array_equal(r[held], np.zeros(held.sum()))
    assert np.array_equal(_bits(z[held]), _bits(eta[held]))
    for u, v in ((w, fb.w), (z, fb.y), (r, fb.r)):
        assert np.array_equal(_bits(u[tr]), _bits(v[tr]))
    miss_t = CL.miss(lab, eta)
    print(f"binomial fold extremes {GX.case_id(case)}: held {int(held.sum())} of which |eta| >= 36 {int((np.abs(eta[held]) >= 36).sum())}, "
          f"misclassified {out[4]:.2f}, held nll off by {abs(out[3] - nll_t[held].sum()) / (U * nll_t[held].sum()):.2f} ulp")
    assert out[4] == miss_t[held].sum() and out[2] == cl_t[tr].sum()
    for got, terms in ((out[0], nll_t[tr]), (out[1], w_t[tr]), (out[3], nll_t[held])):
        assert abs(got - terms.sum()) <= (n + 64) * U * np.abs(terms).sum()
    sw, _ = _wmoments(fa)
    assert abs(sw - w.sum()) <= n * U * w.sum()
    for g in (fa, fb, fc):
        g.close()


# ---- c. the Poisson step -----------------------------------------------------------------------------------------------------------
P_PARAMS = [(em, c) for em in GX.P_ETA_MAX for c in GX.P_CASES[em]]
P_IDS = ["etamax%d-%s" % (em, GX.case_id(c)) for em, c in P_PARAMS]


def _poisson(monkeypatch, eta_max, case):
    n, cap, branch, start = case
    GX.reaches(n, cap, branch)
    tab = GX.P_TABLES[eta_max]
    e = GX.entries(len(tab[0]), n, start)
    eta, cnt, place, lin, off = (t[e] for t in tab)
    return e, eta, cnt, place, lin, off, (lambda: _inject(monkeypatch, cap, lambda X: cd.CDPoissonLoss(cnt, X, off), lin, n + start))


def _poisson_scales(cnt, eta, eta_max, w_t):
    """What a row's rounding errors are relative to (tests/test_gpu_poisson.py's _scales, with the deviance's term for
    |log(y / mu)| beyond 10): (y + mu) / w for r, mu + |y ec| for nll, y |log(y / mu)| + y + mu for dev -- the log is a few ulp
    of itself and its argument a few ulp of y / mu, both times y, and d = y - mu a few ulp of its operands.  dev's scale
    is only used where dev is finite."""
    ec = np.minimum(eta, eta_max)
    mu = np.exp(ec)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        lg = np.where(cnt > 0.0, np.abs(np.log(np.where(cnt > 0.0, cnt, 1.0) / mu)), 0.0)
        s_dev = np.where(cnt > 0.0, cnt * lg, 0.0) + cnt + mu
    return mu, (cnt + mu) / w_t, mu + np.abs(cnt * ec), s_dev


def _poisson_mu(cnt, w, r, cl_t):
    """The device's mu where the outputs hold it: w itself on an unclamped row, -r wmin on a clamped row with count 0."""
    have = ~cl_t | (cnt == 0.0)
    return have, np.where(cl_t, -r * WMIN, w)


@pytest.mark.parametrize("eta_max,case", P_PARAMS, ids=P_IDS)
def test_poisson_step_on_the_table(monkeypatch, eta_max, case):
    """Both APPLY forms, no fold.  Exactly: a row at eta == eta_max is not capped and the next double above it is, the capped
    and the clamped count are the twin's, (w == wmin) is the twin's flag row by row, every capped row and every row at eta_max
    has the same w, z == eta_lin + r, dev == 2 mu on the count-0 rows with the device's own mu, dev == 0 and r == 0 at
    count 1 and eta 0, dev == +inf on every row whose y / mu overflows, the offset-injected and the X-injected rows agree bit for bit in w and r, nll, w, z and r are finite
    everywhere -- count 1e300 at eta 700 included --, and the deviance of the training rows is +inf, not NaN.  Against the
    twin: w at 64 2^-53 relative, r at 64 2^-53 (y + mu) / w, a row's finite dev at 64 2^-53 of its scale (_poisson_scales), the cancellation rows (X beta = 800, o = -800 + c) among them;
    mu by test_device_exp_read_back's bound in spacings where it is subnormal.  Measured on an MI355X: 0.00 ulp on w, r and
    dev in all 16 cases, mu 0 spacings from numpy's."""
    e, eta, cnt, place, lin, off, make = _poisson(monkeypatch, eta_max, case)
    n = len(eta)
    f = make()
    w_t, z_t, r_t, nll_t, dev_t, cl_t, cap_t = PN.rows(cnt, lin, off, WMIN, eta_max)
    mu_t, s_r, s_nll, s_dev = _poisson_scales(cnt, eta, eta_max, w_t)
    inf = dev_t == np.inf
    assert (inf.any() or n < GP.ROWS) and not np.isnan(dev_t).any()      # (a slice of 33 entries may hold no such row)
    rows = [int(i) for i in _first_rows(e)]
    dev = {i: _one_row(f, i, lambda g, k, a: _pstep(g, k, a, eta_max)) for i in rows}      # read-only, before the step
    ro = _pstep(f, -1, 0, eta_max)
    out = _pstep(f, -1, 1, eta_max)
    assert np.array_equal(ro, out)
    w, z, r = f.w, f.y, f.r
    assert np.isfinite(np.r_[w, z, r, out[:5]]).all() and out[4] == 0.0
    if inf.any():
        assert out[5] == np.inf
    else:
        assert abs(out[5] - dev_t.sum()) <= (n + 64) * U * s_dev.sum()
    # exactly
    assert out[3] == cap_t.sum() == (eta > eta_max).sum() and out[2] == cl_t.sum()
    assert np.array_equal(w == WMIN, cl_t) and np.array_equal(z, lin + r)
    top = cap_t | (eta == eta_max)
    assert (w[top] == w[top][0]).all() if top.any() else True
    have, mu = _poisson_mu(cnt, w, r, cl_t)
    worst_dev = 0.0
    for i, o6 in dev.items():
        assert np.isfinite(o6).all() or o6[5] == np.inf, (i, o6)
        if cnt[i] == 0.0:
            assert o6[4] == 2.0 * mu[i], (i, eta[i], o6, mu[i])
        elif cnt[i] == 1.0 and eta[i] == 0.0:
            assert o6[4] == 0.0 and r[i] == 0.0 and w[i] == 1.0, (i, o6, r[i])
        elif inf[i]:
            assert o6[4] == np.inf, (i, eta[i], cnt[i], o6)
        else:
            worst_dev = max(worst_dev, abs(o6[4] - dev_t[i]) / s_dev[i])
    pair = np.flatnonzero((place[:-1] == 0) & (place[1:] == 1) & (e[1:] == e[:-1] + 1))
    assert len(pair) >= 10 and np.array_equal(_bits(w[pair]), _bits(w[pair + 1])) and np.array_equal(_bits(r[pair]), _bits(r[pair + 1]))
    # against the twin
    d, normal = _spacings(mu[have], mu_t[have])
    slack = np.where(cl_t & (cnt == 0.0), EXP_BOUND["subnormal"] * TINY / WMIN, 0.0)
    ew, er = np.abs(w - w_t) / w_t, (np.abs(r - r_t) - slack) / np.maximum(s_r, TINY)
    cancel = place == 2
    print(f"poisson extremes eta_max={eta_max:g} {GX.case_id(case)}: worst ulps w {ew.max() / U:.2f} r {er.max() / U:.2f} "
          f"(cancellation rows: w {ew[cancel].max() / U:.2f} r {er[cancel].max() / U:.2f}) dev {worst_dev / U:.2f}; mu read back on {have.sum()} rows, worst "
          f"spacings {_worst(d, normal)}; clamped {int(out[2])} capped {int(out[3])} rows with dev = inf {int(inf.sum())}")
    assert np.all(ew <= 64 * U) and np.all(er <= 64 * U) and worst_dev <= 64 * U and cancel.sum() >= 10
    assert _exp_ok(d, normal)
    for got, terms, scale in ((out[0], nll_t, s_nll), (out[1], w_t, w_t)):
        assert abs(got - terms.sum()) <= (n + 64) * U * scale.sum()
    f.close()


@pytest.mark.parametrize("side", ("training", "held-out"))
@pytest.mark.parametrize("eta_max,case", P_PARAMS, ids=P_IDS)
def test_poisson_fold_step_on_the_table(monkeypatch, eta_max, case, side):
    """Every row whose deviance is +inf (count > 0 and y / mu overflows) once among the training rows and once among the
    held-out rows, a third of the other rows held out either time.  The side that has them sums to +inf; the other sum is
    finite and within the summation bound of the twin's -- `held ? dev : 0.0` as a product with a 0/1 mask would make it NaN.
    Held-out rows: w == 0, never wmin, r == 0, z the bits of eta_lin; the training rows the plain step's bit for bit;
    the capped count runs over all live rows.  Measured on an MI355X: the finite sum <= 5.68 ulp of its scale."""
    e, eta, cnt, place, lin, off, make = _poisson(monkeypatch, eta_max, case)
    n = len(eta)
    w_t, z_t, r_t, nll_t, dev_t, cl_t, cap_t = PN.rows(cnt, lin, off, WMIN, eta_max)
    mu_t, s_r, s_nll, s_dev = _poisson_scales(cnt, eta, eta_max, w_t)
    inf = dev_t == np.inf
    held = (GX.third(n) & ~inf) if side == "training" else (GX.third(n) | inf)
    tr = ~held
    assert (held & ~inf).any() and (tr & ~inf).any() and (np.abs(eta[held]) >= GX.P_SAT).any()
    assert inf.any() or n < GP.ROWS                          # (a slice of 33 entries may hold no such row: both sums are finite then)
    fa, fb = make(), make()
    fa.set_folds(held.astype(np.int32), 2)
    plain = _pstep(fb, -1, 1, eta_max)
    ro = _pstep(fa, 1, 0, eta_max)
    out = _pstep(fa, 1, 1, eta_max)
    assert np.array_equal(ro, out) and not np.isnan(out).any()
    w, z, r = fa.w, fa.y, fa.r
    assert np.isfinite(np.r_[w, z, r, out[:4]]).all()
    assert np.array_equal(w[held], np.zeros(held.sum())) and np.array_equal(r[held], np.zeros(held.sum()))
    assert np.array_equal(_bits(z[held]), _bits(lin[held]))
    for u, v in ((w, fb.w), (z, fb.y), (r, fb.r)):
        assert np.array_equal(_bits(u[tr]), _bits(v[tr]))
    assert out[3] == plain[3] == cap_t.sum() and out[2] == cl_t[tr].sum()
    with_inf, other, rows_other = (out[5], out[4], held) if side == "training" else (out[4], out[5], tr)
    want = dev_t[rows_other].sum()
    print(f"poisson fold extremes eta_max={eta_max:g} {GX.case_id(case)} inf among the {side} rows: that sum {with_inf}, the other "
          f"{other:.6g} off by {abs(other - want) / max(U * s_dev[rows_other].sum(), TINY):.2f} ulp of its scale; held {int(held.sum())}")
    assert np.isfinite(other)
    if inf.any():
        assert with_inf == np.inf
    else:
        rows_inf = tr if side == "training" else held
        assert abs(with_inf - dev_t[rows_inf].sum()) <= (n + 64) * U * s_dev[rows_inf].sum()
    tiny = 2.0 * EXP_BOUND["subnormal"] * TINY * n            # (dev = 2 mu of the count-0 rows whose mu is subnormal or zero)
    assert abs(other - want) <= (n + 64) * U * s_dev[rows_other].sum() + tiny
    for got, terms, scale in ((out[0], nll_t[tr], s_nll[tr]), (out[1], w_t[tr], w_t[tr])):
        assert abs(got - terms.sum()) <= (n + 64) * U * scale.sum()
    fa.close()
    fb.close()


# ---- d. the device's exp, read back ------------------------------------------------------------------------------------------------
def test_device_exp_read_back(monkeypatch):
    """The device's exp over both tables (n = 513, every entry), from the rows that hold it exactly -- r wmin on the rightly
    classified binomial rows beyond |eta| = 37.5, w on the unclamped Poisson rows, -r wmin on the clamped ones with count 0 --
    against numpy's, in spacings of the result.  numpy is within 1 spacing of mpmath there (tests/test_glm_extremes_host.py);
    the bound is max(measured, 1) + 2.  Measured on an MI355X, 780 rows and 20 arguments from -800 to 700: 1.0 spacings in the
    normal range (at -708.0, where numpy is 0.35 from mpmath), 0.0 in the subnormal range (120 rows)."""
    case = [c for c in GX.B_CASES if c[0] == GP.ROWS + 1][0]
    e, eta, lab, make = _binomial(monkeypatch, case)
    f = make()
    _irls(f, 1)
    _, right, _ = _binomial_masks(eta, lab)
    got, ref, arg = [_binomial_e(eta, f.r, right)[0]], [np.exp(-np.abs(eta[right]))], [-np.abs(eta[right])]
    f.close()
    for em in GX.P_ETA_MAX:
        case = [c for c in GX.P_CASES[em] if c[0] == GP.ROWS + 1][0]
        e, eta, cnt, place, lin, off, make = _poisson(monkeypatch, em, case)
        f = make()
        _pstep(f, -1, 1, em)
        cl_t = PN.rows(cnt, lin, off, WMIN, em)[5]
        have, mu = _poisson_mu(cnt, f.w, f.r, cl_t)
        got.append(mu[have])
        ref.append(np.exp(np.minimum(eta, em))[have])
        arg.append(np.minimum(eta, em)[have])
        f.close()
    got, ref, arg = np.concatenate(got), np.concatenate(ref), np.concatenate(arg)
    d, normal = _spacings(got, ref)
    worst = _worst(d, normal)
    at = {k: float(arg[m][np.argmax(d[m])]) for k, m in (("normal", normal), ("subnormal", ~normal))}
    print(f"device exp read back on {len(got)} rows, {len(np.unique(arg))} arguments from {arg.min():g} to {arg.max():g}: worst distance "
          f"from numpy in spacings {worst} at {at}")
    assert normal.sum() >= 100 and (~normal).sum() >= 100 and len(np.unique(arg)) >= 20
    assert worst["normal"] <= EXP_BOUND["normal"] and worst["subnormal"] <= EXP_BOUND["subnormal"]


# ---- e. solves on hard data ---------------------------------------------------------------------------------------------------------
KINDS = {"default": {}, "cache forced": {"CDH_GRADIENT_CACHE": "3"}, "one-launch": {"CDH_SMALL_PATH": "1"}}


@pytest.mark.parametrize("name", list(GX.SOLVES))
def test_solves_on_hard_data_agree_on_three_kinds_of_handle(monkeypatch, name):
    """Linearly separable labels (|eta| to 34 and 76, 91 and 195 of 300 rows clamped at the solution), exposures sixteen powers
    of e apart (60 rows with mu below wmin from the first step on) and the same counts capped at eta_max = 4 for three rounds
    in which F rises: weights of 1e-5 beside residuals of 1e5 through the weighted lasso on the default handle, the forced
    gradient cache and the one-launch solve.  Inner optTol 1e-12, IRLS optTol 1e-10.  beta against the twin, and every kind
    against every other, at the project's 1e-10; rounds, converged and monotone the twin's; the clamped and capped counts of
    the final read-only step the twin's; the KKT conditions of F in numpy at 1e-8 where the solve converges.  Measured on an
    MI355X, max|beta - twin| on the default handle / the forced cache / the one-launch solve: separable-0.01 7.1e-15 / 7.1e-15 /
    1.2e-14, separable-0.002 1.2e-14 / 1.2e-14 / 1.1e-12, exposures 3.3e-16 / 3.3e-16 / 2.2e-16, exposures-b 1.1e-16 / 1.1e-16 /
    6.7e-16, capped 4.4e-16 / 4.4e-16 / 1.6e-15, capped-b 2.8e-16 / 2.8e-16 / 1.3e-15; KKT <= 9.3e-13."""
    t = GX.twin_solve(name)
    X, y, o, lam, icpt, p = t["X"], t["y"], t["o"], t["lam"], t["icpt"], GX.P_SOLVE
    poisson = t["family"] == "poisson"
    X1 = PN.with_ones(X) if icpt else X
    om = np.r_[np.ones(p), 0.0] if icpt else None
    opts = cd.CDOptions(maxIter=10000, optTol=GX.INNER_TOL, randomize=False)
    irls = cd.IRLSOptions(**t["irls"])
    want = np.r_[t["beta"], t["b0"]] if icpt else t["beta"]
    got = {}
    for kind, env in KINDS.items():
        with monkeypatch.context() as m:                     # read when the handle is made; the suite's own setting comes back
            for k, v in env.items():
                m.setenv(k, v)
            f = cd.CDPoissonLoss(y, X1, o) if poisson else cd.CDLogisticLoss(y, X1)
        x = cd.SparseIterate(X1.shape[1])
        if icpt:
            x[p + 1] = PN.null_intercept(y, o)
        if poisson:
            sol = cd.poissonLasso_(x, f, cd.ProxL1(lam, om), opts, irls)
            last = f.irls_step(False, irls.wmin, irls.etaMax)
            assert sol.capped == last["capped"]
        else:
            sol = cd.logisticLasso_(x, f, cd.ProxL1(lam, om), opts, irls)
            last = dict(f.irls_step(False, irls.wmin), capped=0)
        beta = x.dense()
        got[kind] = beta
        assert np.isfinite(beta).all() and np.isfinite(sol.nll)
        assert (sol.rounds, sol.converged, sol.monotone) == (t["rounds"], t["converged"], t["monotone"]), (kind, sol)
        assert (last["clamped"], last["capped"]) == (t["clamped"], t["capped"]), (kind, last)
        kkt = None
        if t["converged"]:
            b, b0 = (beta[:p], beta[p]) if icpt else (beta, 0.0)
            on, off_, ic = PN.kkt(X, y, o, b, lam, None, b0) if poisson else LG.kkt(X, y, b, lam)
            kkt = max(on, off_, ic if icpt else 0.0)
            assert kkt <= 1e-8, (kind, on, off_, ic)
        print(f"hard solve [{name}, {kind}]: max|beta - twin| {np.max(np.abs(beta - want)):.2e} rounds {sol.rounds} clamped "
              f"{last['clamped']} capped {last['capped']} monotone {sol.monotone} KKT {kkt} onchip {f.onchip_stats()['solves']}")
        if kind == "one-launch":
            assert f.onchip_stats()["solves"] >= t["rounds"]
        else:
            assert f.onchip_stats()["solves"] == 0
        if kind == "cache forced":
            assert f.gradient_cache_mode() == 3
        f.close()
    for kind in KINDS:
        assert np.max(np.abs(got[kind] - want)) <= 1e-10, kind
        for other in KINDS:
            assert np.max(np.abs(got[kind] - got[other])) <= 1e-10, (kind, other)
