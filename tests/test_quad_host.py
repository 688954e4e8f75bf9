"""CDQuadraticLoss without a GPU: the constructor's checks (src/cd_differentiable_function.jl:304-308), which run before the
device is touched, and the host-only arithmetic of the batched solve (csrc/quad_solve_types.hpp: where a problem's state
lies in LDS, CDH_QUAD_MAX_P, the argument checks), compiled with g++ into a stand-alone program with the host sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUDGET = 160 * 1024


def _spd(p, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((2 * p + 2, p))
    return X.T @ X / X.shape[0]


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the arguments were checked")


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(cd._lib, "lib", lambda: _NoDevice())


def test_constructor_refuses_before_any_device_call(no_device):
    A = _spd(5)
    b = np.arange(5.0)
    asym = A.copy()
    asym[0, 1] += 1e-9
    with pytest.raises(cd.ArgumentError, match="symmetric"):
        cd.CDQuadraticLoss(asym, b)
    with pytest.raises(cd.ArgumentError, match="square"):
        cd.CDQuadraticLoss(A[:, :4], b)
    with pytest.raises(cd.ArgumentError, match="length"):
        cd.CDQuadraticLoss(A, b[:4])
    with pytest.raises(cd.ArgumentError, match="length"):
        cd.CDQuadraticLoss(A, np.zeros((4, 3)))
    with pytest.raises(TypeError):
        cd.CDQuadraticLoss(A.astype(np.float32), b.astype(np.float32))
    with pytest.raises(TypeError):
        cd.CDQuadraticLoss(A, b.astype(np.float32))
    with pytest.raises(AssertionError, match="reached"):      # (the guard of this test itself: valid arguments do go on to the device)
        cd.CDQuadraticLoss(A, b)


@pytest.fixture(scope="module")
def layout_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quad") / "quad_layout")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "quad_layout_main.cpp")], check=True)
    return exe


def test_lds_layout_at_the_edges(layout_program):
    P = cd.CDH_QUAD_MAX_P
    sizes = [1, 63, 64, 65, 1024, P, P + 1]
    out = subprocess.run([layout_program] + [str(p) for p in sizes], check=True, capture_output=True, text=True).stdout
    rows = {int(a): (int(b), int(c)) for a, b, c in re.findall(r"^p (\d+) bytes (\d+) fits (\d)$", out, flags=re.M)}
    assert sorted(rows) == sizes                              # every size passed overlap, alignment and bounds (exit status 0)
    for p in sizes[:-1]:
        assert rows[p][1] == 1 and rows[p][0] <= BUDGET, (p, rows[p])
    assert rows[P + 1][1] == 0 and rows[P + 1][0] > BUDGET    # the limit is tight
    assert P >= 1024
    # the three places that name the limit agree: the formula, the Python constant, the C header; the refusal names it
    assert int(re.search(r"^max_p (\d+) budget (\d+)$", out, flags=re.M).group(1)) == P
    assert int(re.search(r"^max_p (\d+) budget (\d+)$", out, flags=re.M).group(2)) == BUDGET
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    assert int(re.search(r"#define CDH_QUAD_MAX_P (\d+)", hdr).group(1)) == P
    assert str(P) in re.search(r"^message (.*)$", out, flags=re.M).group(1)


def test_types_header_holds_no_hip():
    txt = open(os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc", "quad_solve_types.hpp")).read()
    code = re.sub(r"//[^\n]*", "", txt)
    assert not re.search(r"__global__|__device__|__shared__|hip[A-Z_]|threadIdx|blockIdx", code)


def test_every_quad_export_is_bound_and_cited():
    names = [s for s in cd.declared_symbols() if s.startswith("cdh_quad_")]
    assert len(names) == 12
    hdr = open(os.path.join(ROOT, "include", "cdhip.h")).read()
    for name in names:
        before = hdr[: hdr.index("int32_t %s(" % name)]
        comment = before[before.rindex("/*"):]
        assert re.search(r"\.jl:\d+", comment), name


def test_a_batch_crosses_the_abi_column_major(monkeypatch):
    """Problem j's b is column j with leading dimension p, and a per-problem omega likewise, whatever order the caller's arrays have."""
    import ctypes as C
    seen = {}

    def read(ptr, count):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(count,)).copy()

    class Fake:
        def cdh_quad_create(self, out, p, max_batch, device):
            out._obj.value = 1
            return 0

        def cdh_quad_set_b(self, h, m, B, ldb):
            seen["B"], seen["ldb"] = read(B, m * ldb), ldb
            return 0

        def cdh_quad_set_penalty(self, h, lam, om, ldo):
            seen["om"], seen["ldo"] = read(om, 3 * ldo), ldo
            return 0

        def __getattr__(self, name):
            return lambda *a: 0

    monkeypatch.setattr(cd._lib, "lib", lambda: Fake())
    p, m = 5, 3
    A, B = _spd(p), np.arange(15.0).reshape(p, m)             # C order: rows are contiguous
    f = cd.CDQuadraticLoss(A, B)
    assert seen["ldb"] == p and np.array_equal(seen["B"], B.T.ravel())
    om = np.arange(15.0).reshape(p, m) + 1
    f._set_penalties([cd.ProxL1(0.1, om[:, j]) for j in range(m)])
    assert seen["ldo"] == p and np.array_equal(seen["om"], om.T.ravel())
    f._h = None
