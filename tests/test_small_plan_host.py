"""The launch plan of the one-launch solve without a GPU (csrc/small_plan.hpp): compiled with g++ -- through a ctypes shim
against its Python restatement (tests/_small_plan.py), and as a stand-alone program under the host sanitizers -- for every
p the kernel takes and both LDS budgets a runtime may grant (160 KB, or the default 64 KB where it refuses the attribute)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _small_plan as SP

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "coordinatedescent.jl_amd", "csrc")
BUDGETS = (SP.WIDE, SP.DEFAULT)
PS = range(1, SP.MAX_P + 1)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("smallplan") / "libsmallplanshim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "small_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    i64, i32 = C.c_int64, C.c_int32
    for name, args, res in (("sp_c_state_bytes", [i64], i64), ("sp_c_fits", [i64, i64], i32), ("sp_c_ncache", [i64, i64], i32),
                            ("sp_c_lds_bytes", [i64, i64], i64), ("sp_c_unroll", [i64], i32), ("sp_c_ctl_bytes", [], i64),
                            ("sp_c_sup_off", [], i64), ("sp_c_beta_off", [i64], i64), ("sp_c_io_bytes", [i64], i64),
                            ("sp_c_max_p", [], i64), ("sp_c_max_lam", [], i64)):
        getattr(L, name).argtypes, getattr(L, name).restype = args, res
    return L


def test_plan_restated_in_python_is_the_headers(shim):
    assert (shim.sp_c_max_p(), shim.sp_c_max_lam(), shim.sp_c_ctl_bytes()) == (SP.MAX_P, SP.MAX_LAM, SP.CTL_BYTES)
    for p in PS:
        assert shim.sp_c_state_bytes(p) == SP.state_bytes(p) == 68 * p + 8
        assert shim.sp_c_unroll(p) == SP.unroll(p)
        assert (shim.sp_c_sup_off(), shim.sp_c_beta_off(p), shim.sp_c_io_bytes(p)) == SP.io_offsets(p)
        for budget in BUDGETS:
            got = (bool(shim.sp_c_fits(p, budget)), shim.sp_c_ncache(p, budget), shim.sp_c_lds_bytes(p, budget))
            assert got == SP.plan(p, budget), (p, budget)
    for p, budget in ((0, SP.WIDE), (SP.MAX_P + 1, SP.WIDE), (1, 0), (1, 75), (1, 76)):
        got = (bool(shim.sp_c_fits(p, budget)), shim.sp_c_ncache(p, budget), shim.sp_c_lds_bytes(p, budget))
        assert got == SP.plan(p, budget), (p, budget)
    # the figures the kernel's description and the edge cases quote
    assert [SP.ncache(p) for p in (1024, 512, 256, 200)] == [11, 31, 71, 93]


def test_plan_invariants_for_every_p_and_both_budgets(shim):
    for p in PS:
        assert 64 * shim.sp_c_unroll(p) >= p                           # the unrolled loops cover the vector ...
        assert shim.sp_c_unroll(p) == 4 or 64 * shim.sp_c_unroll(p) // 2 < p     # ... with the narrowest kernel that does
        sup, beta, end = shim.sp_c_sup_off(), shim.sp_c_beta_off(p), shim.sp_c_io_bytes(p)
        assert sup % 16 == 0 and beta % 16 == 0                        # 16-byte aligned, and no part overlaps the next
        assert shim.sp_c_ctl_bytes() <= sup and sup + 4 * p <= beta and beta + 8 * p == end
        for budget in BUDGETS:
            fits, nc, lds = bool(shim.sp_c_fits(p, budget)), shim.sp_c_ncache(p, budget), shim.sp_c_lds_bytes(p, budget)
            state = shim.sp_c_state_bytes(p)
            assert fits == (not (budget == SP.DEFAULT and p >= 964)), (p, budget)      # exactly p >= 964 at 64 KB, never at 160 KB
            assert 0 <= nc <= 256
            if fits:
                assert state + nc * 8 * p <= budget and lds == state + nc * 8 * p
                assert nc == 256 or state + (nc + 1) * 8 * p > budget               # and no column is left out that would fit
            else:
                assert (nc, lds) == (0, 0)                              # nothing to launch with: small_prepare switches the path off


def test_the_old_formula_wrapped_where_the_plan_now_refuses():
    """ncache = min(256, (budget - state) / 8p) in size_t: at 64 KB and p >= 964 the subtraction wrapped to 256 columns and
    ~2 MB of LDS.  The restatement of that arithmetic, to show what the plan's `fits` replaces."""
    for p in (963, 964, 1024):
        state = SP.state_bytes(p)
        wrapped = min(256, ((SP.DEFAULT - state) % (1 << 64)) // (8 * p))
        fits, nc, lds = SP.plan(p, SP.DEFAULT)
        if p < 964:
            assert fits and wrapped == nc == 0 and lds == state <= SP.DEFAULT
        else:
            assert wrapped == 256 and state + wrapped * 8 * p > 30 * SP.DEFAULT and not fits


def test_sanitized_stand_alone_program(tmp_path):
    exe = str(tmp_path / "small_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "small_plan_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "small_plan_main OK" in out


def test_plan_header_holds_no_hip_and_the_library_has_no_second_copy():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "small_plan.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|hip[A-Z_]|threadIdx|blockIdx", code)
    for name in ("small_solve.hpp", "cdhip.hip"):
        txt = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        assert "struct SmallCtl" not in txt and "9 * sizeof(int32_t)" not in txt and "size_t small_sup_off" not in txt, name
        assert not re.search(r"p <= (256|512)\b", txt), name                 # the unroll thresholds are small_unroll's
    txt = open(os.path.join(CSRC, "small_solve.hpp")).read()
    assert "small_plan(h->p, budget)" in txt and "small_unroll(h->p)" in txt
    assert re.search(r"if \(!plan\.fits\) \{ sp\.enabled = false; return CDH_OK; \}", txt)
