"""cdh_vc_gram_batch without a GPU: the plan of a call (csrc/vc_gram_batch_types.hpp) compiled with g++ -- through a ctypes
shim against its Python restatement (tests/_vc_gram_batch_plan.py), and as a stand-alone program under the host sanitizers;
the batch argument check; and what the front ends do on the host: broadcasting, their errors, the chunking of long point
lists, the stacked solve against the per-point one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _vc_gram_batch_plan as BP
import _vc_gram_numpy as VG

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NS, QS, MBS = [1, 64, 65, 32768, 32769, 10 ** 6], [0, 1, 2, 3], [1, 3, 4, 64]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vcgrambatch") / "libvcgrambatchshim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "vc_gram_batch_shim.cpp")], check=True)
    L = C.CDLL(so)
    i64, i32, f64, P = C.c_int64, C.c_int32, C.c_double, C.POINTER
    for name, args, res in (("vgb_c_resident", [i64, i32, i64], i32), ("vgb_c_chunks", [i64], i64), ("vgb_c_grid", [i64, i32, i64], i64),
                            ("vgb_c_group_points", [i64, i32, i64], i64), ("vgb_c_groups", [i64, i32, i64, i64], i64),
                            ("vgb_c_group_first", [i64, i32, i64, i64], i64), ("vgb_c_group_size", [i64, i32, i64, i64, i64], i64),
                            ("vgb_c_share_points", [i64, i32, i64, i64], i64), ("vgb_c_grid_y", [i64, i32, i64, i64], i64),
                            ("vgb_c_share_begin", [i64, i32, i64, i64, i64], i64), ("vgb_c_rec_offset", [i64, i32, i64, i64, i64], i64),
                            ("vgb_c_device_bytes", [], i64), ("vgb_c_pinned_bytes", [], i64), ("vgb_c_point_bytes", [], i64),
                            ("vgb_c_check", [i32, i32, i32, i64, i64, i32, i64, P(f64), P(f64), P(i64), i32, i64, P(i64), P(i64)],
                             C.c_char_p)):
        getattr(L, name).argtypes, getattr(L, name).restype = args, res
    return L


def _ms(pg):
    return [m for m in (1, 2, pg - 1, pg, pg + 1, BP.K["kVgbMaxPoints"]) if 1 <= m <= BP.K["kVgbMaxPoints"]]


def test_plan_restated_in_python_is_the_headers(shim):
    for n in NS:
        for Q in QS:
            for mb in MBS:
                pg = shim.vgb_c_group_points(n, Q, mb)
                assert pg == BP.plan(n, Q, mb, 1)["group_points"]
                for m in _ms(pg):
                    pl = BP.plan(n, Q, mb, m)
                    assert pl["resident"] == bool(shim.vgb_c_resident(n, Q, mb)) and pl["G"] == shim.vgb_c_grid(n, Q, mb)
                    assert len(pl["groups"]) == shim.vgb_c_groups(n, Q, mb, m)
                    for g, grp in enumerate(pl["groups"]):
                        pts = grp["pts"]
                        assert (grp["first"], pts) == (shim.vgb_c_group_first(n, Q, mb, g), shim.vgb_c_group_size(n, Q, mb, m, g))
                        assert (grp["per"], grp["grid_y"]) == (shim.vgb_c_share_points(n, Q, mb, pts), shim.vgb_c_grid_y(n, Q, mb, pts))
                        for s in {0, 1, grp["grid_y"] // 2, grp["grid_y"] - 1, grp["grid_y"]}:
                            assert grp["edges"][s] == shim.vgb_c_share_begin(n, Q, mb, pts, s), (n, Q, mb, m, g, s)
                        for point, block in ((0, 0), (pts - 1, pl["G"] - 1), (pts // 2, pl["G"] // 2)):
                            assert BP.rec_offset(n, Q, mb, point, block) == shim.vgb_c_rec_offset(n, Q, mb, point, block)
    assert BP.K["kVgbMaxPoints"] == cd.CDH_VC_GRAM_MAX_POINTS == 65536
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    assert int(re.search(r"#define CDH_VC_GRAM_MAX_POINTS (\d+)", hdr).group(1)) == 65536
    point = shim.vgb_c_point_bytes()
    assert point == 24
    assert shim.vgb_c_device_bytes() == 8 * (BP.K["kVgbPartialDoubles"] + BP.K["kVgbOutDoubles"]) + point * BP.K["kVgbMaxGroupPoints"]
    assert shim.vgb_c_pinned_bytes() == 8 * BP.K["kVgbOutDoubles"] + point * BP.K["kVgbMaxGroupPoints"]
    assert BP.K["kVgbPartialDoubles"] == 1 << 24                     # partial records: at most 2^24 doubles (128 MiB)


def test_plan_invariants_over_the_sweep():
    """Every point is in exactly one group and one share, the groups' records fit the partial buffer, and the regime
    switches exactly where the single-point deal gives a workgroup more than one chunk."""
    seen = set()
    for n in NS:
        for Q in QS:
            for mb in MBS:
                la = VG.launch(n, Q, mb)
                pg = BP.plan(n, Q, mb, 1)["group_points"]
                assert pg >= 8
                for m in _ms(pg):
                    pl = BP.plan(n, Q, mb, m)
                    assert pl["resident"] == (not la["wraps"]) == (la["chunks"] <= la["G"])
                    covered = 0
                    for grp in pl["groups"]:
                        assert grp["first"] == covered and 1 <= grp["pts"] <= pg
                        assert grp["pts"] * pl["G"] * pl["nrec"] <= BP.K["kVgbPartialDoubles"]
                        assert grp["pts"] * pl["nrec"] <= BP.K["kVgbOutDoubles"] and 1 <= grp["grid_y"] <= 65535
                        e = grp["edges"]
                        assert e[0] == 0 and e[-1] == grp["pts"] and all(a < b for a, b in zip(e, e[1:]))     # no empty share
                        if pl["resident"]:
                            assert grp["grid_y"] == 1 or grp["per"] >= BP.K["kVgbMinSharePoints"]
                            assert (grp["grid_y"] - 1) * pl["G"] < BP.K["kVgbTargetBlocks"]
                        else:
                            assert grp["per"] == 1 and grp["grid_y"] == grp["pts"]
                        covered += grp["pts"]
                    assert covered == m
                    seen.add((pl["resident"], len(pl["groups"]) > 1))
    assert seen == {(True, False), (True, True), (False, False), (False, True)}
    assert BP.plan(32768, 1, 3, 1)["resident"] and not BP.plan(32769, 1, 3, 1)["resident"]     # 512 chunks, and one more
    assert not BP.plan(32768, 3, 64, 1)["resident"]                  # the largest record: the partial buffer caps the grid earlier


def test_every_refusal_of_the_batch_check_names_its_point(shim):
    idx = np.array([3, 1, 3], dtype=np.int64)
    m = 5

    def msg(m=m, h=None, z0="default", lo="default", deg=1, y_set=1, want_c=1, kind=0, wpow=1, mb=3, idx=idx, no_h=False):
        hh = np.full(5, 0.3) if h is None else np.asarray(h, dtype=np.float64)
        zz = np.linspace(0.0, 1.0, 5) if isinstance(z0, str) else z0
        ll = np.array([-1, 1, -1, 9, -1], dtype=np.int64) if isinstance(lo, str) else lo
        bad = C.c_int64(99)
        p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))     # noqa: E731
        out = shim.vgb_c_check(deg, y_set, want_c, 3, 10, kind, m, None if no_h else p(hh, C.c_double), p(zz, C.c_double),
                               p(ll, C.c_int64), wpow, mb, p(idx, C.c_int64), C.byref(bad))
        return out, bad.value

    assert msg() == (None, -1)                                       # a mixed batch: plain points, left-out rows
    assert msg(h=[0.1, 0.2, 0.3, 0.4, 0.5], lo=None) == (None, -1) and msg(kind=1, wpow=2, y_set=0, want_c=0) == (None, -1)
    assert msg(z0=None, lo=np.arange(5, dtype=np.int64)) == (None, -1)
    for kw, word, point in ((dict(m=0), b"65536", -1), (dict(m=65537), b"65536", -1), (dict(no_h=True), b"bandwidth", -1),
                            (dict(idx=None), b"base_idx1", -1), (dict(z0=None), b"z0", 0), (dict(z0=None, lo=None), b"z0", 0),
                            (dict(z0=None, lo=np.array([0, 1, 2, -1, 4], dtype=np.int64)), b"z0", 3),
                            (dict(h=[0.3, 0.3, 0.0, 0.3, 0.3]), b"bandwidth", 2), (dict(h=[0.3, 0.3, 0.3, 0.3, np.nan]), b"bandwidth", 4),
                            (dict(z0=np.array([0.0, 0.1, np.inf, 0.3, 0.4])), b"z0", 2),
                            (dict(lo=np.array([-1, 10, -1, 9, -1], dtype=np.int64)), b"row", 1),
                            (dict(lo=np.array([-1, 1, -1, 9, -2], dtype=np.int64)), b"row", 4),
                            (dict(deg=-1), b"cdh_vc_set_data", 0), (dict(y_set=0), b"cdh_set_y", 0), (dict(kind=2), b"kernel", 0),
                            (dict(wpow=3), b"wpow", 0), (dict(mb=0), b"mb", 0), (dict(mb=65), b"mb", 0),
                            (dict(idx=np.array([3, 0, 3], dtype=np.int64)), b"p_base", 0)):
        out, bad = msg(**kw)
        assert word in (out or b"") and bad == point, (kw, out, bad)
    # a non-finite z0 where the point leaves a row out is not read as a point
    assert msg(z0=np.array([0.0, np.nan, 0.2, np.inf, 0.4])) == (None, -1)


def test_sanitized_stand_alone_program(tmp_path):
    exe = str(tmp_path / "vc_gram_batch_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "vc_gram_batch_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "vc_gram_batch_main OK" in out


def test_batch_types_header_holds_no_hip():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(VG.CSRC, "vc_gram_batch_types.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|hip[A-Z_]|threadIdx|blockIdx", code)


def test_the_export_is_declared_bound_and_cited():
    assert "cdh_vc_gram_batch" in cd.declared_symbols()
    assert len(cd._lib.lib().cdh_vc_gram_batch.argtypes) == 13
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    before = hdr[: hdr.index("int32_t cdh_vc_gram_batch(")]
    comment = before[before.rindex("/*"):]
    for lines in ("217-235", "348-380", "383-409", "572-647"):
        assert lines in comment, lines
    txt = open(os.path.join(VG.CSRC, "vc_gram.hpp")).read()
    assert re.search(r"void k_vc_moments\(", txt) and "varying_coefficient_lasso.jl:217-235" in txt


# ---- the front ends on the host ------------------------------------------------------------------------------------------
class _FakeLoss(cd.CDVaryingCoefficientLoss):
    """A loss without a handle: expanded_gram_batch's own host code runs up to the library call, which records its arguments."""

    def __init__(self, n=20, p_base=2, degree=1):
        self.n, self.p_base, self.degree, self.p, self.dtype = n, p_base, degree, p_base * (degree + 1), np.dtype(np.float64)
        self._h, self.calls = None, []

        class L:
            pass
        self._L = L()
        self._L.cdh_vc_gram_batch = self._record

    def _record(self, h, kind, m, *rest):
        self.calls.append((kind, m))
        return cd._lib.CDH_OK

    def close(self):
        pass

    __del__ = close


def test_expanded_gram_batch_broadcasts_and_refuses_on_the_host():
    f = _FakeLoss()
    G, c, sw = f.expanded_gram_batch(cd.GaussianKernel, 0.3, np.linspace(0, 1, 7))
    assert G.shape == (7, 4, 4) and c.shape == (7, 4) and sw.shape == (7,) and f.calls[-1] == (0, 7)
    G, c, sw = f.expanded_gram_batch(cd.EpanechnikovKernel(0.1), [0.3, 0.4, 0.5], leave_out=[0, -1, 19], z0=0.5, rhs=False)
    assert G.shape == (3, 4, 4) and c is None and f.calls[-1] == (1, 3)
    assert f.expanded_gram_batch(1, 0.3, 0.5, base_cols=[1])[0].shape == (1, 2, 2)          # all scalars: one point
    with pytest.raises(cd.DimensionMismatch):
        f.expanded_gram_batch(cd.GaussianKernel, [0.3, 0.4], [0.1, 0.2, 0.3])
    with pytest.raises(cd.DimensionMismatch):
        f.expanded_gram_batch(cd.GaussianKernel, [0.3, 0.4], 0.5, leave_out=[1, 2, 3])
    with pytest.raises(cd.DimensionMismatch):
        f.expanded_gram_batch(cd.GaussianKernel, 0.3, [0.5, 0.6], e=np.ones(19))
    for bad in (dict(h=np.ones((2, 2)), z0=0.5), dict(h=0.3, z0=np.zeros((3, 1))), dict(h=0.3, leave_out=np.zeros((2, 2), dtype=int)),
                dict(h=0.3, leave_out=[0.5, 1.0])):
        with pytest.raises(TypeError):
            f.expanded_gram_batch(cd.GaussianKernel, **bad)
    for k in ("gaussian", cd.SmoothingKernel, None, True):
        with pytest.raises(TypeError):
            f.expanded_gram_batch(k, 0.3, 0.5)
    n_calls = len(f.calls)
    with pytest.raises(cd.ArgumentError, match="65536"):
        f.expanded_gram_batch(cd.GaussianKernel, 0.3, np.zeros(65537))
    with pytest.raises(cd.ArgumentError):
        f.expanded_gram_batch(cd.GaussianKernel, np.zeros(0), 0.5)
    assert len(f.calls) == n_calls                                   # refused before the library, and before any allocation


def test_front_ends_cut_long_point_lists_into_modest_calls(monkeypatch):
    """70 000 grid points are more than one call takes: locpoly sends them in pieces of at most 4096."""
    f = _FakeLoss(n=20, p_base=1, degree=0)
    sizes = []
    real = cd.CDVaryingCoefficientLoss.expanded_gram_batch

    def spy(self, kernel, h, z0=None, **kw):
        G, c, sw = real(self, kernel, h, z0, **kw)
        sizes.append(G.shape[0])
        G[:] = 1.0                                                   # (a solvable system: 1 x = t)
        c[:, 0] = z0
        return G, c, sw

    monkeypatch.setattr(cd.CDVaryingCoefficientLoss, "expanded_gram_batch", spy)
    zgrid = np.arange(70000.0)
    out = cd.locpoly(f, None, None, zgrid, None, cd.GaussianKernel(0.3))
    assert out.shape == (1, 70000) and np.array_equal(out[0], zgrid)
    assert sum(sizes) == 70000 and max(sizes) == 4096 and sizes[:-1] == [4096] * 17


def test_stacked_solve_is_the_per_point_solve():
    """_solve_scaled_stack applies _solve_scaled's scaling to every block; LAPACK sees the same systems one by one."""
    from coordinatedescent_jl_amd import api
    rng = np.random.default_rng(4)
    A = rng.standard_normal((9, 30, 6))
    G = np.einsum("tij,tik->tjk", A, A)
    c = rng.standard_normal((9, 6))
    got = api._solve_scaled_stack(G.transpose(0, 2, 1), c)
    for t in range(9):
        assert got[t].tobytes() == api._solve_scaled(np.asfortranarray(G[t]), c[t]).tobytes()
