"""The Cox step on the device: cdh_glm_set_survival, cdh_glm_get_survival, cdh_glm_cox_irls (k_cox_exp -> k_cox_offsets ->
k_cox_scan -> k_cox_hazard -> k_cox_offsets -> k_cox_scan -> k_cox_apply -> k_gram_reduce), held row by row to the numpy twin
(tests/_cox_numpy.py; its two forms and its gradient are pinned in tests/test_cox_plan_host.py) at the eta the handle held.

The scans' scratch is NOT exported: S, A and B are checked through w, r, z and the record, whose bounds follow from theirs.
With U = 2^-53, the twin's math.fsum values taken as exact, and every scanned sum made of positive terms:
    |dS| <= (n + 8) U S,  |dA| <= (2n + 16) U A,  |dB| <= (3n + 16) U B          (not observable here)
    w (unclamped)   |dw| <= (5n + 64) U eA
    d = delta - eA  |dd| <= (2n + 64) U (delta + eA)
    r               |dr| <= (|dd| bound + |r| |dw| bound) / w
    z               |dz| <= |dr| bound + U |eta_lin|
    a record sum    (n + 64) U sum |terms|: the terms are w for sum w and delta (log S - eta) >= 0 for the nll
The nll's bound is relative to the terms themselves, and a term can be all rounding: the latest event of a distinct-time
problem is its own risk set, S = e, and log(exp(eta)) - eta is 0 up to the roundings of exp and log.  Where such terms are
the whole sum (n = 1, 2) the bound (n + 64) U sum |terms| is a few ulp of nothing and cannot be met by any implementation whose
exp or log differs from the twin's in the last bit.  So the nll is held to that bound wherever it is at least NLL_FLOOR, and
to NLL_FLOOR above it elsewhere:  NLL_FLOOR = sum over the events of (n + 8) U + 2 U |log S| -- S carries a relative error of
up to (n + 8) U into log S, the library's log is within an ulp (2 U |log S|); eta itself has the twin's bits.  Every case prints
the multiple of the plain bound too, floor or not, and LAB_NOTES.md "Cox lasso" lists the cases that miss it.
Every case prints the worst measured multiple of its bounds; LAB_NOTES.md "Cox lasso" holds the ones seen on an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cox_numpy as CX
import _cox_plan as CP

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OK, BAD = cd._lib.CDH_OK, cd._lib.CDH_BAD_ARG
T = CP.TILE
WMIN, EMAX = 1e-5, 1.5                       # eta_max = 1.5: the rows above it cap

# (n, grid cap, ties, offset, presorted)
NS = [(n, CP.MAX_GRID) for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)] + [(5 * T + 3, 2)]
CASES = []
for n_, cap_ in NS:
    CASES += [(n_, cap_, "distinct", True, False), (n_, cap_, "rounded", False, True)]
for n_, cap_ in ((T + 1, CP.MAX_GRID), (5 * T + 3, 2)):
    CASES += [(n_, cap_, "rounded", True, False), (n_, cap_, "distinct", False, True)]
for n_, cap_ in ((65, CP.MAX_GRID), (2 * T + 1, CP.MAX_GRID), (5 * T + 3, 2)):
    CASES += [(n_, cap_, "equal", True, False), (n_, cap_, "early", False, False), (n_, cap_, "late", True, True)]
IDS = ["n%d-cap%d-%s-%s-%s" % (n, cap, ties, "off" if o else "nooff", "sorted" if s else "random") for n, cap, ties, o, s in CASES]


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _data(n, ties, with_offset, presorted):
    """Times: distinct; rounded so that a few dozen tie groups span the rows; all equal; and distinct times whose events lie
    only among the earliest tenth of the rows, or only among the latest tenth."""
    rng = np.random.default_rng(1000 + n)
    X = np.asfortranarray(rng.standard_normal((n, 3)))
    t = rng.exponential(1.0, n)
    status = (rng.random(n) < 0.7).astype(np.float64)
    if ties == "rounded":
        t = np.round(t, 1)
    elif ties == "equal":
        t[:] = 2.5
    elif ties in ("early", "late"):
        cut = np.quantile(t, 0.1 if ties == "early" else 0.9)
        status = ((t <= cut) if ties == "early" else (t >= cut)).astype(np.float64) * status
    if not status.any():
        status[int(np.argmin(t)) if ties != "late" else int(np.argmax(t))] = 1.0
    off = rng.uniform(-0.5, 0.5, n) if with_offset else None
    if presorted:
        o = np.argsort(t, kind="stable")
        X, t, status = np.asfortranarray(X[o]), t[o], status[o]
        off = None if off is None else off[o]
    x = cd.SparseIterate(3)
    x[1], x[2], x[3] = 0.8, -0.6, 0.4
    return X, t, status, off, x


def _loss(monkeypatch, t, status, X, off=None, cap=CP.MAX_GRID):
    if cap != CP.MAX_GRID:
        monkeypatch.setenv("CDH_COX_GRID", str(cap))            # read when the handle is made
    return cd.CDCoxLoss(np.c_[t, status], X, off)


def _step(f, k, apply, wmin=WMIN, eta_max=EMAX):
    out = np.zeros(5)
    cd.check(f._L.cdh_glm_cox_irls(f._h, int(k), int(apply), float(wmin), float(eta_max), out.ctypes.data_as(C.POINTER(C.c_double))),
             f._h)
    return out


def _wmoments(f):
    sw, swr2 = C.c_double(), C.c_double()
    cd.check(f._L.cdh_resid_wmoments(f._h, C.byref(sw), C.byref(swr2)), f._h)
    return sw.value, swr2.value


def _moments(f):
    s1, s2 = C.c_double(), C.c_double()
    cd.check(f._L.cdh_resid_moments(f._h, C.byref(s1), C.byref(s2)), f._h)
    return s1.value, s2.value


def _pads_are_zero(f, n, w, z, r):
    """The pad rows n .. ld - 1 of w, r and y through sums the library takes over all ld rows: sum w and sum w r^2, sum r and
    sum r^2, and -- after initialize! at beta = 0, which makes r a copy of y, pads included -- the same two sums of y.  Each is
    held to the n real rows' own sum within n U of its absolute terms, so a pad row that holds anything but zero shows unless
    it is below the rounding of the sum.  Leaves the handle at beta = 0 with its y and w."""
    sw, swr2 = _wmoments(f)
    assert abs(sw - w.sum()) <= n * U * w.sum() and abs(swr2 - (w * r * r).sum()) <= 2 * n * U * max((w * r * r).sum(), 1e-300)
    for v in (r, z):
        if v is z:
            f._synced = None
            cd.initialize_(f, cd.SparseIterate(f.p))
        s1, s2 = _moments(f)
        assert abs(s1 - math.fsum(v)) <= n * U * max(np.abs(v).sum(), 1e-300), (v is z, s1, math.fsum(v))
        assert abs(s2 - math.fsum(v * v)) <= 2 * n * U * max((v * v).sum(), 1e-300), (v is z, s2)


def _straddles(t, n, cap):
    """Does a tie group cross a wave's, a tile's, a workgroup's boundary (in sorted positions)?"""
    _, first, last = CX.groups(t)
    pl = CP.plan(CP.padded(n), cap)
    wave = np.any(first // 256 != last // 256)
    tile = np.any(first // T != last // T)
    edges = [CP.run_first(pl["tiles"], pl["grid"], b) * T for b in range(1, pl["grid"])]
    wg = any(np.any((first < e) & (last >= e)) for e in edges)
    return wave, tile, wg


def _check_rows(tag, n, w, z, r, out, q, eta_lin, train, wmin):
    """w, z, r and the record against the twin's exact rows q, by the bounds of the module's docstring.  -> nothing; prints
    the worst multiples."""
    tr = np.ones(n, dtype=bool) if train is None else train
    unc = tr & ~q["clamped"]
    scale_d = q["delta"] + q["eA"]
    bw = (5 * n + 64) * U * q["eA"]
    bd = (2 * n + 64) * U * scale_d
    br = (bd + np.abs(q["r"]) * bw) / np.where(tr, q["w"], 1.0)
    bz = br + U * np.abs(eta_lin)
    mw = (np.abs(w - q["w"])[unc] / bw[unc]).max() if unc.any() else 0.0
    nz = tr & (br > 0.0)
    mr = (np.abs(r - q["r"])[nz] / br[nz]).max() if nz.any() else 0.0
    mz = (np.abs(z - q["z"])[nz] / bz[nz]).max() if nz.any() else 0.0
    ev = q["delta"] != 0.0
    s_w = float(q["w"][tr].sum())
    m_sw = abs(out[1] - s_w) / ((n + 64) * U * s_w)
    # the nll: the plain bound (n + 64) U sum |terms| where it is not degenerate, the floor of the module's docstring on top of it elsewhere
    err_nll = abs(out[0] - math.fsum(q["nll"][tr]))
    plain = (n + 64) * U * math.fsum(np.abs(q["nll"][tr]))
    floor = math.fsum((n + 8) * U + 2 * U * np.abs(np.log(q["S"][ev])))
    degenerate = plain < floor
    m_plain = err_nll / plain if plain > 0.0 else (0.0 if err_nll == 0.0 else np.inf)
    m_nll = err_nll / (plain + floor) if degenerate else m_plain
    print(f"cox step {tag}: worst multiples of the bounds: w {mw:.3f} r {mr:.3f} z {mz:.3f} nll {m_nll:.3f} sum_w {m_sw:.3f}; "
          f"nll against (n + 64) U sum|terms| alone: {m_plain:.3f}{' (DEGENERATE: below the floor, held to bound + floor)' if degenerate else ''}; "
          f"clamped {int(out[2])} capped {int(out[3])} events {int(out[4])}")
    assert mw <= 1.0 and mr <= 1.0 and mz <= 1.0 and m_nll <= 1.0 and m_sw <= 1.0
    # exact facts: the clamped rows hold wmin itself; rows where the bound is zero (A = 0: before the first event) hold r = 0
    np.testing.assert_array_equal(w[tr & q["clamped"]], wmin)
    np.testing.assert_array_equal(r[tr & (br == 0.0)], 0.0)
    assert out[2] == q["clamped"][tr].sum() and out[3] == q["capped"].sum() and out[4] == q["delta"].sum()
    before = tr & (q["A"] == 0.0)
    np.testing.assert_array_equal(w[before], wmin)
    np.testing.assert_array_equal(r[before], 0.0)


def _twin(eta_lin, off, t, status, train=None, wmin=WMIN, emax=EMAX):
    q = CX.rows(eta_lin, off, t, status, wmin, emax, train, exact=True)
    q["off"], q["emax"] = off, emax
    return q


# ---- the step, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,ties,with_offset,presorted", CASES, ids=IDS)
def test_step_row_by_row(monkeypatch, n, cap, ties, with_offset, presorted):
    X, t, status, off, x = _data(n, ties, with_offset, presorted)
    wave, tile, wg = _straddles(t, n, cap)
    if ties in ("rounded", "equal"):
        # tie groups across every kind of boundary the shape has (from 2 tiles up one boundary lies where the times are dense)
        assert wave == (n > 256) and (tile and wg) == (n > 2 * T or (ties == "equal" and n > T))
    f = _loss(monkeypatch, t, status, X, off, cap)
    np.testing.assert_array_equal(f.time, t)
    np.testing.assert_array_equal(f.status, status)
    np.testing.assert_array_equal(f.offset, np.zeros(n) if off is None else off)
    np.testing.assert_array_equal(f.y, np.zeros(n))
    cd.initialize_(f, x)
    eta_lin = f.y - f.r                                          # what the kernels recover, from the same two stored vectors
    assert n < 60 or np.max(np.abs(eta_lin)) > 1.0
    q = _twin(eta_lin, off, t, status)
    ro = _step(f, -1, 0)
    out = _step(f, -1, 1)
    assert np.array_equal(ro, out)                               # the read-only form takes the same sums, bit for bit
    w, z, r = f.w, f.y, f.r
    _check_rows(IDS[CASES.index((n, cap, ties, with_offset, presorted))], n, w, z, r, out, q, eta_lin, None, WMIN)
    assert n < 60 or ties in ("early", "late", "equal") or (out[3] > 0 and out[2] < n)      # some rows cap, not every row clamps
    # apply = 0 changes no bit of w, y, r; the data are where they were
    _step(f, -1, 0)
    for a, b in ((f.w, w), (f.y, z), (f.r, r)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(f.time, t)
    np.testing.assert_array_equal(f.status, status)
    # the pad rows of w, r and y were written as zeros (n = 63, 65, T +- 1, 2 T + 1, 5 T + 3 have some)
    _pads_are_zero(f, n, w, z, r)
    f.close()


def test_sums_are_exact_at_the_null_model(monkeypatch):
    """beta = 0, no offset, all times equal, every row an event, n a power of two: e = 1, S = n, A = 1, B = 1 / n, so
    w = 1 - 1 / n and r = 0 EXACTLY on every row, sum w == n - 1, nll == n log n within the sum's bound, events == n, whatever
    the order of the scans' additions.  (These n have no pad rows: those are the next test's.)"""
    for n, cap in ((64, CP.MAX_GRID), (T, CP.MAX_GRID), (4 * T, 2)):
        rng = np.random.default_rng(n)
        X = np.asfortranarray(rng.integers(-3, 4, size=(n, 2)).astype(np.float64))
        f = _loss(monkeypatch, np.full(n, 3.0), np.ones(n), X, None, cap)
        for apply in (0, 1, 1):
            out = _step(f, -1, apply, 1e-5, 50.0)
            assert out[1:].tolist() == [float(n - 1), 0.0, 0.0, float(n)], (n, apply, out)
            assert abs(out[0] - n * np.log(n)) <= (n + 64) * U * n * np.log(n)
        np.testing.assert_array_equal(f.w, np.full(n, 1.0 - 1.0 / n))
        np.testing.assert_array_equal(f.r, np.zeros(n))
        np.testing.assert_array_equal(f.y, np.zeros(n))
        assert _wmoments(f) == (float(n - 1), 0.0)
        np.testing.assert_array_equal(cd.stdX(f, weighted=True), np.sqrt((X * X).sum(axis=0) * (1.0 - 1.0 / n) / n))
        f.close()


@pytest.mark.parametrize("n", (40, T + 8))
def test_pad_rows_are_zero_where_every_row_is_known_exactly(monkeypatch, n):
    """n is no multiple of 32, so the handle has 24 pad rows.  beta = 0, no offset, all times equal and ONE event: e = 1 and
    S = n exactly, A = fl(1 / n) and B = fl(A / n) are sums of one term, so every row has w = fl(A - B), r = fl((delta - A) / w)
    and z = r to the bit, whatever the order of the scans; the sums over all ld rows then show the pads of w, r and y."""
    rng = np.random.default_rng(n)
    X = np.asfortranarray(rng.integers(-3, 4, size=(n, 2)).astype(np.float64))
    status = np.zeros(n)
    status[n // 3] = 1.0
    f = _loss(monkeypatch, np.full(n, 3.0), status, X, None)
    assert CP.padded(n) - n == 24
    A = 1.0 / n
    B = A / n
    w_t = np.full(n, A - B)
    r_t = (status - A) / w_t
    for apply in (0, 1):
        out = _step(f, -1, apply, 1e-5, 50.0)
        assert out[2:].tolist() == [0.0, 0.0, 1.0] and abs(out[0] - np.log(n)) <= 2 * U * np.log(n)
        assert abs(out[1] - n * (A - B)) <= (n + 64) * U * n * (A - B)
    w, z, r = f.w, f.y, f.r
    np.testing.assert_array_equal(w, w_t)
    np.testing.assert_array_equal(r, r_t)
    np.testing.assert_array_equal(z, r_t)
    _pads_are_zero(f, n, w, z, r)
    f.close()


def test_repeatable_and_blind_to_folds_at_k_minus_one(monkeypatch):
    """Two identical steps on two handles are bit-identical; so is k = -1 with folds set."""
    n, cap = 5 * T + 3, 2
    X, t, status, off, x = _data(n, "rounded", True, False)
    got = []
    for folds in (False, False, True):
        f = _loss(monkeypatch, t, status, X, off, cap)
        if folds:
            f.set_folds(np.arange(n) % 3, 3)
        cd.initialize_(f, x)
        ro = _step(f, -1, 0)
        out = _step(f, -1, 1)
        got.append((ro, out, f.w, f.y, f.r))
        f.close()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            np.testing.assert_array_equal(a, b)


# ---- folds -------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [c for c in CASES if c[0] >= 63 and c[2] in ("distinct", "rounded")][::2]
assert (5 * T + 3, 2, "rounded", True, False) in FOLD_CASES and (T + 1, CP.MAX_GRID, "distinct", True, False) in FOLD_CASES
FOLD_IDS = [IDS[CASES.index(c)] for c in FOLD_CASES]


@pytest.mark.parametrize("n,cap,ties,with_offset,presorted", FOLD_CASES, ids=FOLD_IDS)
def test_fold_rows_leave_the_risk_sets(monkeypatch, n, cap, ties, with_offset, presorted):
    """With fold k held out: held rows get w = 0, r = 0 and z = eta exactly; the training rows agree, within the bounds of the
    plain step, with the twin evaluated on the training rows ALONE."""
    X, t, status, off, x = _data(n, ties, with_offset, presorted)
    ids = np.random.default_rng(n).permutation(n) % 3
    k = 1
    train = ids != k
    if not status[train].any():
        status = status.copy()
        status[np.nonzero(train)[0][0]] = 1.0
    f = _loss(monkeypatch, t, status, X, off, cap)
    f.set_folds(ids, 3)
    cd.initialize_(f, x)
    eta_lin = f.y - f.r
    q = _twin(eta_lin, off, t, status, train)
    alone = CX.rows(eta_lin[train], None if off is None else off[train], t[train], status[train], WMIN, EMAX, None, exact=True)
    for key in ("w", "r", "z"):
        np.testing.assert_array_equal(q[key][train], alone[key])  # (the twin's own statement of "the training rows alone")
    ro = _step(f, k, 0)
    out = _step(f, k, 1)
    assert np.array_equal(ro, out)
    w, z, r = f.w, f.y, f.r
    np.testing.assert_array_equal(w[~train], 0.0)
    np.testing.assert_array_equal(r[~train], 0.0)
    np.testing.assert_array_equal(z[~train], eta_lin[~train])
    _check_rows("fold " + FOLD_IDS[FOLD_CASES.index((n, cap, ties, with_offset, presorted))], n, w, z, r, out, q, eta_lin, train, WMIN)
    _pads_are_zero(f, n, w, z, r)
    f.close()


# ---- the handle's other lives, and the refusals ----------------------------------------------------------------------------------
def test_a_cox_handle_turns_binomial_again(monkeypatch):
    """After a Cox step, cdh_glm_set_labels makes the handle a binomial one whose step equals a fresh handle's bit for bit;
    and the other steps refuse a Cox handle, as the Cox step refuses theirs."""
    n = T + 1
    X, t, status, off, x = _data(n, "rounded", True, False)
    labels = (np.random.default_rng(0).random(n) < 0.5).astype(np.float64)
    f = _loss(monkeypatch, t, status, X, off)
    cd.initialize_(f, x)
    _step(f, -1, 1)
    L, h = f._L, f._h
    out3, out6 = np.zeros(3), np.zeros(6)
    po = C.POINTER(C.c_double)
    assert L.cdh_glm_irls(h, 1, 1e-5, out3.ctypes.data_as(po)) == BAD
    assert L.cdh_glm_poisson_irls(h, -1, 1, 1e-5, 50.0, out6.ctypes.data_as(po)) == BAD
    cd.check(L.cdh_glm_set_labels(h, 0, _vp(labels)), h)
    assert L.cdh_glm_cox_irls(h, -1, 1, 1e-5, 50.0, out6.ctypes.data_as(po)) == BAD
    assert L.cdh_glm_get_survival(h, _vp(out6), None) == BAD
    g = cd.CDLogisticLoss(labels, X)
    f._synced = None
    for u in (f, g):
        cd.initialize_(u, x)
    a, b = np.zeros(3), np.zeros(3)
    cd.check(L.cdh_glm_irls(h, 1, 1e-5, a.ctypes.data_as(po)), h)
    cd.check(g._L.cdh_glm_irls(g._h, 1, 1e-5, b.ctypes.data_as(po)), g._h)
    np.testing.assert_array_equal(a, b)
    for u, v in ((f.w, g.w), (f.y, g.y), (f.r, g.r)):
        np.testing.assert_array_equal(u, v)
    # ... and a Cox handle again, by the export, with its earlier buffers
    cd.check(L.cdh_glm_set_survival(h, _vp(t), _vp(status), None), h)
    np.testing.assert_array_equal(f.time, t)
    np.testing.assert_array_equal(f.offset, np.zeros(n))
    f.close()
    g.close()


def test_refusals_leave_the_handle_unchanged(monkeypatch):
    n = 65
    X, t, status, off, x = _data(n, "rounded", True, False)
    f = _loss(monkeypatch, t, status, X, off)
    cd.initialize_(f, x)
    before = _step(f, -1, 0)
    L, h = f._L, f._h
    po = C.POINTER(C.c_double)
    out = np.zeros(5)

    def refused(status_code, word=None):
        assert status_code == BAD
        assert len(L.cdh_last_error(h)) > 0
        if word is not None:
            assert word.encode() in L.cdh_last_error(h), L.cdh_last_error(h)

    bad = t.copy()
    bad[7] = np.nan
    refused(L.cdh_glm_set_survival(h, _vp(bad), _vp(status), None), "time[7]")
    bad = status.copy()
    bad[9] = 0.5
    refused(L.cdh_glm_set_survival(h, _vp(t), _vp(bad), None), "status[9]")
    bad = off.copy()
    bad[3] = np.inf
    refused(L.cdh_glm_set_survival(h, _vp(t), _vp(status), _vp(bad)), "offset[3]")
    refused(L.cdh_glm_set_survival(h, _vp(t), _vp(np.zeros(n)), None), "no row is an event")
    refused(L.cdh_glm_set_survival(h, None, _vp(status), None))
    refused(L.cdh_glm_set_survival(h, _vp(t), None, None))
    refused(L.cdh_glm_get_survival(h, None, None))
    for args in ((-1, 2, 1e-5, 50.0), (-1, 1, 0.0, 50.0), (-1, 1, 1e-5, 0.0), (-1, 1, 1e-5, 701.0), (-2, 1, 1e-5, 50.0),
                 (0, 1, 1e-5, 50.0)):
        refused(L.cdh_glm_cox_irls(h, *args, out.ctypes.data_as(po)))
    refused(L.cdh_glm_cox_irls(h, -1, 1, 1e-5, 50.0, None), "out5")
    for code in (L.cdh_glm_set_survival(None, _vp(t), _vp(status), None), L.cdh_glm_get_survival(None, _vp(t), None),
                 L.cdh_glm_cox_irls(None, -1, 1, 1e-5, 50.0, out.ctypes.data_as(po))):
        assert code == BAD
    np.testing.assert_array_equal(f.time, t)
    np.testing.assert_array_equal(f.status, status)
    np.testing.assert_array_equal(f.offset, off)
    assert np.array_equal(_step(f, -1, 0), before)
    f.close()
