"""cdh_vc_gram and the locpoly front ends without a GPU: the yardstick of the GPU tests (tests/_vc_gram_numpy.py) pinned to the
reference's own test "expand_X multiplications" (test/varying_coefficient_lasso.jl:68-92) through a restatement of the
_expand_Xt_w_X! / _expand_Xt_w_Y! loops (src/varying_coefficient_lasso.jl:572-647) and to the Kronecker identity; the
host-only arithmetic of csrc/vc_gram_types.hpp (record layout, scatter, launch split, argument checks) compiled with g++ --
through a ctypes shim, and as a stand-alone program under the host sanitizers; and what the front ends do on the host:
their type and dimension errors, get_beta!, getResiduals!."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _vc_gram_numpy as VG
from _vc_numpy import expand, weights

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the yardstick ---------------------------------------------------------------------------------------------------
def loops_Xt_w_X(w, X, z, z0, degree):
    """_expand_Xt_w_X! (:572-620) as the reference runs it: for every pair of base columns j <= k and every row, the running
    products v1 = X[i, j] w[i] df^jj and v2 = X[i, k] df^kk fill the lower triangle of the block; then the mirror."""
    n, p = X.shape
    Q1 = degree + 1
    out = np.zeros((p * Q1, p * Q1))
    for j in range(p):
        for k in range(j, p):
            for i in range(n):
                v1 = X[i, j] * w[i]
                df = z[i] - z0
                for jj in range(Q1):
                    v2 = X[i, k]
                    if k != j:
                        krange = range(Q1)
                    else:
                        krange = range(jj, Q1)
                        v2 = v2 * df ** jj
                    for kk in krange:
                        out[k * Q1 + kk, j * Q1 + jj] += v2 * v1
                        v2 *= df
                    v1 *= df
    low = np.tril(out)
    return low + np.tril(out, -1).T


def loops_Xt_w_Y(w, X, z, y, z0, degree):
    """_expand_Xt_w_Y! (:622-647)."""
    n, p = X.shape
    Q1 = degree + 1
    out = np.zeros(p * Q1)
    for j in range(p):
        for i in range(n):
            v = X[i, j] * w[i] * y[i]
            df = z[i] - z0
            for jj in range(Q1):
                out[j * Q1 + jj] += v
                v *= df
    return out


@pytest.fixture(scope="module")
def ref_case():
    rng = np.random.default_rng(68)
    X = np.asfortranarray(rng.standard_normal((100, 10)))
    return X, rng.random(100), rng.standard_normal(100)


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_yardstick_matches_the_reference_loops(ref_case, degree):
    X, z, y = ref_case
    w = weights("gaussian", 0.2, z, 0.5)
    G, c, sw, aG, ac = VG.gram(X, z, y, 0.5, degree, "gaussian", 0.2)
    u = 2.0 ** -53
    assert np.all(np.abs(loops_Xt_w_X(w, X, z, 0.5, degree) - G.astype(np.float64)) <= (100 + 2 * degree + 4) * u * aG.astype(np.float64))
    assert np.all(np.abs(loops_Xt_w_Y(w, X, z, y, 0.5, degree) - c.astype(np.float64)) <= (100 + degree + 4) * u * ac.astype(np.float64))
    assert abs(float(sw) - w.sum()) <= 100 * u * w.sum()
    # ... and the reference's own assertions: eX' Diagonal(w) Y and (eX' Diagonal(w)) eX
    eX = expand(X, z, 0.5, degree)
    np.testing.assert_allclose(G.astype(np.float64), (eX.T * w) @ eX, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(c.astype(np.float64), eX.T @ (w * y), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_yardstick_expansion_is_the_kronecker_product(ref_case, degree):
    X, z, _ = ref_case
    cols = [7, 2, 2, 9]
    eX = VG.expanded(X, z, 0.5, degree, cols)
    d = z - 0.5
    for i in (0, 17, 99):
        want = np.kron(X[i, cols].astype(VG.LD), np.array([VG.LD(d[i]) ** l for l in range(degree + 1)]))
        assert np.all(np.abs(eX[i] - want) <= 4 * np.finfo(VG.LD).eps * np.abs(want))


def test_yardstick_weights_powers_and_left_out_row(ref_case):
    X, z, y = ref_case
    e = np.arange(100.0)
    om = VG.omega("epanechnikov", 0.4, z, float(z[5]), wpow=2, e=e, leave_out=5)
    w = weights("epanechnikov", 0.4, z, float(z[5]))
    assert om[5] == 0 and w[5] == 0.75 / 0.4
    keep = np.arange(100) != 5
    assert np.array_equal(om[keep], w[keep].astype(VG.LD) ** 2 * e[keep])
    G, c, sw, _, _ = VG.gram(X, z, y, None, 1, "epanechnikov", 0.4, leave_out=5)
    G2, c2, sw2, _, _ = VG.gram(X[keep], z[keep], y[keep], float(z[5]), 1, "epanechnikov", 0.4)     # the reference deletes the row
    assert np.allclose(G.astype(float), G2.astype(float), rtol=1e-15) and np.allclose(c.astype(float), c2.astype(float), rtol=1e-15)


# ---- csrc/vc_gram_types.hpp through a shim -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vcgram") / "libvcgramshim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "vc_gram_shim.cpp")], check=True)
    L = C.CDLL(so)
    i64, i32, f64, P = C.c_int64, C.c_int32, C.c_double, C.POINTER
    for name, args, res in (("vg_nrec", [i32, i64], i64), ("vg_tri", [i64, i64, i64], i64), ("vg_off_m", [i32, i64], i64),
                            ("vg_off_w", [i32, i64], i64), ("vg_pairs", [i64], i32), ("vg_slices", [i64], i32),
                            ("vg_grid", [i64, i32, i64], i32), ("vg_chain", [i64, i32, i64], i64),
                            ("vg_scatter", [i32, i64, P(f64), P(f64), P(f64)], None),
                            ("vg_check", [i32, i32, i32, i64, i64, i32, f64, f64, i64, i32, i64, P(i64)], C.c_char_p)):
        getattr(L, name).argtypes, getattr(L, name).restype = args, res
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.parametrize("Q", [0, 1, 2, 3])
@pytest.mark.parametrize("mb", [1, 2, 3, 64])
def test_scatter_puts_every_moment_where_the_expanded_order_wants_it(shim, Q, mb):
    """Moment matrices whose entries encode (s, j, k): a wrong index is a wrong number."""
    Q1, ep, n = Q + 1, mb * (Q + 1), shim.vg_nrec(Q, mb)
    assert n == VG.nrec(Q, mb)
    rec = np.full(n, np.nan)
    M = np.zeros((2 * Q + 1, mb, mb))
    m = np.zeros((Q1, mb))
    for s in range(2 * Q + 1):
        for j in range(mb):
            for k in range(j, mb):
                M[s, j, k] = M[s, k, j] = 1e6 * (s + 1) + 1e3 * (j + 1) + (k + 1)
                rec[s * (mb * (mb + 1) // 2) + shim.vg_tri(mb, j, k)] = M[s, j, k]
    for a in range(Q1):
        for j in range(mb):
            m[a, j] = -(1e3 * (a + 1) + j + 1)
            rec[shim.vg_off_m(Q, mb) + a * mb + j] = m[a, j]
    rec[shim.vg_off_w(Q, mb)] = 0.5
    assert not np.isnan(rec).any() and shim.vg_off_w(Q, mb) == n - 1          # no gaps: every entry of the record was written
    G, c = np.full((ep, ep), np.nan, order="F"), np.full(ep, np.nan)
    shim.vg_scatter(Q, mb, _dp(rec), _dp(G), _dp(c))
    jj, aa = np.divmod(np.arange(ep), Q1)
    assert np.array_equal(G, M[aa[:, None] + aa[None, :], jj[:, None], jj[None, :]])
    assert np.array_equal(c, m[aa, jj]) and np.array_equal(G, G.T)


def test_every_refusal_of_the_argument_check(shim):
    idx = np.array([3, 1, 3], dtype=np.int64)
    good = dict(deg=1, y_set=1, want_c=1, p_base=3, n=10, kind=0, h=0.5, z0=0.1, lo=-1, wpow=1, mb=3)

    def msg(**kw):
        a = dict(good, **kw)
        return shim.vg_check(a["deg"], a["y_set"], a["want_c"], a["p_base"], a["n"], a["kind"], a["h"], a["z0"], a["lo"],
                             a["wpow"], a["mb"], idx.ctypes.data_as(C.POINTER(C.c_int64)))

    assert msg() is None and msg(kind=1, wpow=2, lo=9, y_set=0, want_c=0) is None
    for kw, word in ((dict(deg=-1), b"cdh_vc_set_data"), (dict(y_set=0), b"cdh_set_y"), (dict(mb=0), b"mb"), (dict(mb=65), b"mb"),
                     (dict(p_base=2), b"p_base"), (dict(h=0.0), b"bandwidth"), (dict(h=-1.0), b"bandwidth"),
                     (dict(h=float("nan")), b"bandwidth"), (dict(kind=2), b"kernel"), (dict(kind=-1), b"kernel"),
                     (dict(wpow=0), b"wpow"), (dict(wpow=3), b"wpow"), (dict(lo=10), b"row"), (dict(lo=-2), b"row"),
                     (dict(z0=float("inf")), b"z0")):
        assert word in (msg(**kw) or b""), kw
    idx[1] = 0
    assert b"p_base" in msg()


def test_launch_arithmetic_restated_in_python_is_the_headers(shim):
    R, B = VG.K["kVgRows"], VG.K["kVgMaxBlocks"]
    for Q in range(4):
        for mb in (1, 2, 3, 4, 5, 10, 14, 15, 62, 63, 64):
            assert shim.vg_pairs(mb) * shim.vg_slices(mb) <= VG.K["kVgThreads"]
            for n in (1, R - 1, R, R + 1, 5 * R + 7, 4099, B * R, B * R + 1, 65537, 10 ** 6):
                la = VG.launch(n, Q, mb)
                assert (la["G"], la["L"], la["pairs"], la["S"]) == (shim.vg_grid(n, Q, mb), shim.vg_chain(n, Q, mb),
                                                                    shim.vg_pairs(mb), shim.vg_slices(mb)), (Q, mb, n)
                assert la["G"] * VG.nrec(Q, mb) <= VG.K["kVgPartialDoubles"]
    assert VG.K["kVgMaxCols"] == cd.CDH_VC_GRAM_MAX_COLS == 64
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    assert int(re.search(r"#define CDH_VC_GRAM_MAX_COLS (\d+)", hdr).group(1)) == 64


def test_the_kernel_header_states_the_chain_length_the_tests_mirror():
    txt = open(os.path.join(VG.CSRC, "vc_gram.hpp")).read()
    assert "// L = ceil(nchunks / G) * ceil(kVgRows / S) + S + ceil(G / 4) + 2" in txt


def test_sanitized_stand_alone_program(tmp_path):
    exe = str(tmp_path / "vc_gram_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "vc_gram_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "vc_gram_main OK" in out


def test_types_header_holds_no_hip():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(VG.CSRC, "vc_gram_types.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|hip[A-Z_]|threadIdx|blockIdx", code)


def test_the_export_is_declared_bound_and_cited():
    assert "cdh_vc_gram" in cd.declared_symbols()
    assert len(cd._lib.lib().cdh_vc_gram.argtypes) == 12
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    before = hdr[: hdr.index("int32_t cdh_vc_gram(")]
    comment = before[before.rindex("/*"):]
    assert "varying_coefficient_lasso.jl:572-620" in comment and ":622-647" in comment


# ---- the front ends on the host ------------------------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the arguments were checked")


def test_front_ends_refuse_bad_types_and_dimensions_before_any_device_call(monkeypatch):
    monkeypatch.setattr(cd._lib, "lib", lambda: _NoDevice())
    rng = np.random.default_rng(0)
    X, z, y = rng.standard_normal((20, 3)), rng.random(20), rng.standard_normal(20)
    k = cd.GaussianKernel(0.3)
    for call in (lambda X, z, y: cd.locpoly(X, z, y, 0.5, 1, k),
                 lambda X, z, y: cd.locpoly(X, z, y, np.linspace(0.1, 0.9, 3), 1, k),
                 lambda X, z, y: cd.lvocv_locpoly(X, z, y, 1, [0.3], cd.GaussianKernel),
                 lambda X, z, y: cd.split_locpoly(X, z, y, X, z, y, np.linspace(0, 1, 3), 1, [0.3], cd.GaussianKernel),
                 lambda X, z, y: cd.refit_locpolyl1(X, z, y, 0.5, 1, k, np.ones(6))):
        with pytest.raises(TypeError):
            call(X.astype(np.float32), z, y)
        with pytest.raises(TypeError):
            call(X, z, y.astype(np.float32))
        with pytest.raises(TypeError):
            call(X[:, 0], z, y)
        with pytest.raises(cd.DimensionMismatch):
            call(X, z[:19], y)
        with pytest.raises(cd.DimensionMismatch):
            call(X, z, y[:19])
        with pytest.raises(AssertionError, match="reached"):         # (the guard of this test: valid arguments do go on)
            call(X, z, y)
    with pytest.raises(TypeError):
        cd.locpoly(X, z, y, 0.5, 1, "gaussian")
    with pytest.raises(TypeError):
        cd.locpoly(X, z, y, 0.5, 1.0, k)
    with pytest.raises(TypeError):
        cd.lvocv_locpoly(X, z, y, 1, [0.3], cd.SmoothingKernel)
    with pytest.raises(TypeError):
        cd.getStandardError(X, z, 1.0, 0.5, 1, None)
    with pytest.raises(cd.DimensionMismatch):
        cd.getStandardErrorHEW(X, z[:3], y, 0.5, 1, k)
    with pytest.raises(cd.ArgumentError, match="64"):
        cd.locpoly(np.zeros((20, 65)), z, y, 0.5, 1, k)


def test_get_beta_keeps_the_references_interpolation_weights():
    zgrid = np.array([0.0, 1.0, 3.0])
    B = np.array([[1.0, 10.0, 100.0], [2.0, 20.0, 200.0]])
    out = np.zeros(2)
    assert np.array_equal(cd.get_beta_(out, zgrid, B, 1.0), [10.0, 20.0]) and out is cd.get_beta_(out, zgrid, B, 0.0)
    assert np.array_equal(cd.get_beta_(out, zgrid, B, 3.0), [100.0, 200.0])
    # between 1 and 3 at z0 = 1.5: α = (1.5 - 1) / (3 - 1) = 0.25 multiplies the LEFT column (id1), 0.75 the right one --
    # by hand 0.25 * 10 + 0.75 * 100 = 77.5 (a textbook interpolation would give 0.75 * 10 + 0.25 * 100 = 32.5)
    assert np.array_equal(cd.get_beta_(out, zgrid, B, 1.5), [77.5, 155.0])
    assert np.array_equal(cd.get_beta_(out, zgrid, B, 0.25), [0.25 * 1 + 0.75 * 10, 0.25 * 2 + 0.75 * 20])
    for z0 in (-0.1, 3.5):
        with pytest.raises(IndexError):
            cd.get_beta_(out, zgrid, B, z0)


def test_get_residuals_against_a_numpy_restatement():
    rng = np.random.default_rng(3)
    n, p, degree = 40, 3, 2
    X, z, y = rng.standard_normal((n, p)), rng.random(n), rng.standard_normal(n)
    zgrid = np.linspace(0.0, 1.0, 6)
    B = rng.standard_normal((p * (degree + 1), 6))
    e = cd.getResiduals_(np.zeros(n), X, z, y, zgrid, B, degree, cd.GaussianKernel(1.0))
    for i in range(n):
        l = np.searchsorted(zgrid, z[i], side="right") - 1
        a = (z[i] - zgrid[l]) / (zgrid[l + 1] - zgrid[l])
        b = a * B[:, l] + (1 - a) * B[:, l + 1]
        assert abs(e[i] - (y[i] - X[i] @ b[::degree + 1])) <= 1e-13
    with pytest.raises(cd.DimensionMismatch):
        cd.getResiduals_(np.zeros(n), X, z, y, zgrid, B[:-1], degree)
    with pytest.raises(cd.DimensionMismatch):
        cd.getResiduals_(np.zeros(n - 1), X, z, y, zgrid, B, degree)
