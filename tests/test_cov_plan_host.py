"""The launch plan and the two layouts of the device pass loop without a GPU (csrc/cov_plan.hpp): compiled with g++ -- through a
ctypes shim against the transcription of what cov_solve() and cs_alloc computed before the header existed (tests/_cov_plan.py),
and as a stand-alone program under the host sanitizers -- for both LDS budgets a runtime may grant (134 KB, or 36 KB of the
default 64 KB where it refuses the attribute)."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

import _cov_plan as CP

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "coordinatedescent.jl_amd", "csrc")
FIELDS = ("why", "ucap", "lds_bytes", "tcap", "nhelp", "big", "full_cap", "fold_limit", "nnz_limit")
NNZS = list(range(0, 201)) + [1375, 1376, 1377]
LAYOUT_PS = (1, 16, 17, 255, 256, 257, 1024, 5600, 100003)
TC = CP.TABLE_CAP
# what cs_alloc carved out of the device scratch, in its order: member of CovSolveBufs -> (element bytes, elements)
DEV = lambda p: dict(
    [(m, (8, p)) for m in "gx bfold bsnap hs newval qs tv pendv ubeta uom ugx uk poff voff uprev iota".split()] +
    [(m, (4, p)) for m in "touched s2i i2s list vb moved holes fills gxp upos aidx occ".split()] +
    [(m, (1, p)) for m in "setflag inmoved forced".split()] + [("colmax", (8, p))] +
    [("Gc", (8, TC * TC)), ("gxc", (8, TC)), ("cidk", (8, TC)), ("gxe", (4, TC))] +
    [(m, (4, p)) for m in "cidof ucid newc".split()] + [("crew", (CP.CREW_BYTES, 1)), ("g_snap", (8, p))])
PIN = lambda p: dict([("in_sup", (4, p)), ("out_sup_idx", (4, p)), ("out_moved_idx", (4, p)), ("out_list", (4, p)),
                      ("out_sup_val", (8, p)), ("out_moved_val", (8, p))])
PER_LAUNCH = ("g", "Gcols", "slot", "a", "omega", "beta")      # cov_solve() fills these itself, launch by launch


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("covplan") / "libcovplanshim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "cov_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    i64, i32, s = C.c_int64, C.c_int32, C.c_char_p
    for name, args, res in (("cp_c_const", [s], i64), ("cp_c_tri_doubles", [i64], i64), ("cp_c_lds_bytes", [i32], i64), ("cp_c_ucap", [i64], i32),
                            ("cp_c_plans", [i64, i32, i32, i64, i32, i32, i32, i64, i64, C.POINTER(i64), C.POINTER(i64)], None),
                            ("cp_c_dev_bytes", [i64], i64), ("cp_c_pin_bytes", [i64], i64), ("cp_c_dev_offset", [i64, s], i64),
                            ("cp_c_pin_offset", [i64, s], i64)):
        getattr(L, name).argtypes, getattr(L, name).restype = args, res
    return L


def plans(shim, p, full, rand, budget, ucap_limit, helpers, big, support_limit=4000, nnzs=NNZS):
    arr, out = (C.c_int64 * len(nnzs))(*nnzs), (C.c_int64 * (9 * len(nnzs)))()
    shim.cp_c_plans(p, full, rand, budget, ucap_limit, helpers, big, support_limit, len(nnzs), arr, out)
    return [dict(zip(FIELDS, out[9 * i:9 * i + 9])) for i in range(len(nnzs))]


def plan1(shim, nnz, p=1000, full=0, rand=0, budget=CP.WIDE, ucap_limit=0, helpers=31, big=0, support_limit=4000):
    return plans(shim, p, full, rand, budget, ucap_limit, helpers, big, support_limit, [nnz])[0]


def test_constants_and_lds_arithmetic_are_the_parents(shim):
    for name, want in (("kCsThreads", 256), ("kCsLdsBudget", CP.WIDE), ("kCsLdsFallback", CP.FALLBACK), ("kCsUcapMax", CP.UCAP_MAX),
                       ("kCsTrackedMargin", CP.TRACKED_MARGIN), ("kCsTableCap", CP.TABLE_CAP), ("kCsTableMargin", CP.TABLE_MARGIN),
                       ("kCsTableLds", CP.TABLE_LDS), ("kCsTrackedBytes", CP.TRACKED_BYTES), ("kCsTrackedSlack", 8),
                       ("kCsShuffleMaxP", CP.SHUFFLE_MAX_P), ("kCsCrewMax", CP.CREW_MAX),
                       ("sizeof(CovSolveCtl)", CP.CTL_BYTES), ("sizeof(CsCrew)", CP.CREW_BYTES)):
        assert shim.cp_c_const(name.encode()) == want, name
    for u in range(0, 400):
        assert shim.cp_c_tri_doubles(u) == CP.tri_doubles(u) and shim.cp_c_lds_bytes(u) == CP.lds_bytes(u) == 4 * u * (u + 1) + 92 * u
    for budget in list(range(0, 160 * 1024, 509)) + [CP.WIDE, CP.FALLBACK, CP.lds_bytes(172) - 1, CP.lds_bytes(172), 1 << 30]:
        assert shim.cp_c_ucap(budget) == CP.ucap_of(budget), budget
    # by value, each beside the arithmetic it follows from
    fits = lambda budget: max(u for u in range(8, CP.UCAP_MAX + 1, 4) if CP.lds_bytes(u) <= budget)
    assert shim.cp_c_ucap(CP.WIDE) == fits(CP.WIDE) == 172 and shim.cp_c_ucap(CP.FALLBACK) == fits(CP.FALLBACK) == 84
    assert CP.lds_bytes(172) == 134848 <= CP.WIDE < CP.lds_bytes(176) == 140800 and 8 * CP.tri_doubles(176) == 124608   # 176: 122 KB for the block alone
    assert CP.lds_bytes(84) == 36288 <= CP.FALLBACK < CP.lds_bytes(88)
    assert 24 * (CP.SHUFFLE_MAX_P + 1) <= CP.lds_bytes(172) and CP.lds_bytes(172) - 24 * (CP.SHUFFLE_MAX_P + 1) == 424
    assert CP.tri_doubles(172) >= CP.TABLE_LDS > CP.tri_doubles(84)


def test_plan_is_the_parents_over_the_cross_product(shim):
    n = 0
    for budget, ucap_limit, helpers, big, full, rand, p in itertools.product(
            (CP.WIDE, CP.FALLBACK), (0, 8, 16, 40, 172, 500), (0, 1, 31, 64), (0, 1), (0, 1), (0, 1), (16, 17, 1000, 5599, 5600, 5601, 100003)):
        got = plans(shim, p, full, rand, budget, ucap_limit, helpers, big)
        for nnz, g in zip(NNZS, got):
            want = CP.plan(p, nnz, full, rand, budget, ucap_limit, helpers, big, 4000)
            assert {k: g[k] for k in want} == want, (budget, ucap_limit, helpers, big, full, rand, p, nnz, g, want)
            n += 1
    assert n == 2 * 6 * 4 * 2 * 2 * 2 * 7 * 204
    for lim in (0, 100, 1375, 1376, 1377, 1 << 40):           # the cache's own limit on the support
        for nnz in (0, 100, 101, 1376):
            g = plan1(shim, nnz, support_limit=lim)
            assert g["nnz_limit"] == min(lim, 1376) and g["why"] == CP.RUN


def test_plan_edges_by_value(shim):
    ucap_w, ucap_f = CP.ucap_of(CP.WIDE), CP.ucap_of(CP.FALLBACK)
    margin = CP.TRACKED_MARGIN
    assert (plan1(shim, 10)["ucap"], plan1(shim, 10, budget=CP.FALLBACK)["ucap"]) == (ucap_w, ucap_f) == (172, 84)
    assert (plan1(shim, 10)["lds_bytes"], plan1(shim, 10, budget=CP.FALLBACK)["lds_bytes"]) == (134848, 36288)
    # helpers come once nnz + margin / 2 > ucap - margin
    first = ucap_w - margin - margin // 2 + 1
    assert first == 137
    a, b = plan1(shim, first - 1), plan1(shim, first)
    assert (a["nhelp"], a["big"], a["full_cap"]) == (0, 0, ucap_w - margin) and (b["nhelp"], b["big"], b["full_cap"]) == (31, 1, CP.INT_MAX)
    assert plan1(shim, first, helpers=500)["nhelp"] == CP.CREW_MAX == 64
    # without helpers a full pass stays in the loop up to ucap - margin coordinates
    assert ucap_w - margin == 148
    a, b = plan1(shim, 148, full=1, helpers=0), plan1(shim, 149, full=1, helpers=0)
    assert (a["why"], a["full_cap"], a["big"]) == (CP.RUN, 148, 1) and (b["why"], b["full_cap"]) == (CP.FULL_BEYOND_CAP, 148)
    assert plan1(shim, 149, full=0, helpers=0)["why"] == CP.RUN
    # CDH_CS_UCAP=16: margin 4, helpers from 11 coordinates on
    assert [plan1(shim, nnz, ucap_limit=16)["nhelp"] for nnz in (10, 11)] == [0, 31] and 11 + 4 // 2 > 16 - 4 >= 10 + 4 // 2
    # a handle whose list outgrew the block once stays with the large instantiation
    assert (plan1(shim, 10)["big"], plan1(shim, 10, big=1)["big"]) == (0, 1)
    # the fallback budget has no room for table mode: no table, no helpers, lists up to ucap - margin
    assert CP.tri_doubles(ucap_f) < CP.TABLE_LDS
    g = plan1(shim, ucap_f - margin, budget=CP.FALLBACK, big=1)
    assert (g["why"], g["tcap"], g["nhelp"], g["big"]) == (CP.RUN, 0, 0, 0) and ucap_f - margin == 60
    assert plan1(shim, 61, budget=CP.FALLBACK)["why"] == CP.LIST_DOES_NOT_FIT
    assert plan1(shim, 10)["tcap"] == CP.TABLE_CAP == 1536
    # a shuffle's six (p + 1)-sized int32 arrays overlay the dynamic LDS
    p_last = CP.lds_bytes(ucap_w) // 24 - 1
    assert p_last == 5617 and p_last >= CP.SHUFFLE_MAX_P
    assert [plan1(shim, 10, p=p, rand=1)["why"] for p in (5600, 5601, 5617, 5618, 100003)] == [CP.RUN] * 3 + [CP.SHUFFLE_DOES_NOT_FIT] * 2
    assert plan1(shim, 10, p=5618, rand=0)["why"] == CP.RUN
    assert [plan1(shim, 10, p=p, rand=1, budget=CP.FALLBACK)["why"] for p in (1511, 1512)] == [CP.RUN, CP.SHUFFLE_DOES_NOT_FIT] and 36288 // 24 - 1 == 1511
    # the table's rows less the margin for entering coordinates
    cap = CP.TABLE_CAP - CP.TABLE_MARGIN
    assert cap == 1376
    assert [plan1(shim, nnz)["why"] for nnz in (cap, cap + 1)] == [CP.RUN, CP.SUPPORT_BEYOND_TABLE]
    assert plan1(shim, cap)["nnz_limit"] == cap
    # a fold beyond max(16, 120000 / p) pending moves is the host's
    assert [plan1(shim, 10, p=p)["fold_limit"] for p in (16, 1000, 7500, 7501, 100003)] == [7500, 120, 16, 16, 16]


def test_layouts_are_the_parents(shim):
    for p in LAYOUT_PS:
        assert shim.cp_c_dev_bytes(p) == CP.dev_bytes(p), p
        assert shim.cp_c_pin_bytes(p) == CP.pin_bytes(p), p
        for members, offset, total, head in ((DEV(p), shim.cp_c_dev_offset, CP.dev_bytes(p), 0),
                                             (PIN(p), shim.cp_c_pin_offset, CP.pin_bytes(p), CP.CTL_BYTES)):
            spans, end = [], -(-head // 256) * 256
            for name, (esz, count) in members.items():
                off = offset(p, name.encode())
                assert off == end, (p, name, off, end)                  # the parent's order, each array on the next 256 bytes
                assert off % 256 == 0 and off + esz * count <= total
                spans.append((off, off + esz * count))
                end = off + -(-esz * count // 256) * 256
            assert end == total
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))  # pairwise disjoint (they are in ascending order)
        assert shim.cp_c_pin_offset(p, b"ctl") == 0
        for name in PIN(p):                                             # the carve of the device scratch leaves the pinned views alone
            assert shim.cp_c_dev_offset(p, name.encode()) == -1


def test_every_pointer_of_the_kernels_buffers_has_a_home():
    txt = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(CSRC, "cov_solve_types.hpp")).read(), flags=re.S)
    body = re.search(r"struct CovSolveBufs \{(.*?)\n\};", txt, flags=re.S).group(1)
    pointers = [n for stmt in body.split(";") if "*" in stmt for n in re.findall(r"\*\s*(\w+)", stmt)]
    assert len(pointers) == len(set(pointers)) == 53
    assert sorted(pointers) == sorted(list(DEV(1)) + list(PIN(1)) + list(PER_LAUNCH))
    # ... and the header's one list names each scratch array once
    code = open(os.path.join(CSRC, "cov_plan.hpp")).read()
    listed = re.findall(r"\bof\(b\.(\w+),", code)
    assert listed == list(DEV(1))


def test_sanitized_stand_alone_program(tmp_path):
    exe = str(tmp_path / "cov_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cov_plan_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "cov_plan_main OK" in out


MOVED = ("kCsThreads", "kCsLdsBudget", "kCsLdsFallback", "kCsUcapMax", "kCsTrackedMargin", "kCsTableCap", "kCsTableMargin", "kCsTableLds",
         "kCsTrackedBytes", "kCsShuffleMaxP", "cs_tri_doubles", "cs_lds_bytes", "cs_ucap", "cs_align")
GONE = ("cs_enabled", "cs_big", "cs_helpers", "cs_shuffle_ok", "cs_lds_budget", "cs_dev", "cs_pin", "cs_pin_dev", "cs_bufs", "cs_ctl",
        "cs_in_sup", "cs_out_sup_idx", "cs_out_moved_idx", "cs_out_list", "cs_out_sup_val", "cs_out_moved_val", "d_colmax", "cs_old",
        "cs_tepoch", "cs_ticks", "n_cs_launches", "n_cs_passes", "n_cs_folds", "n_cs_exact", "n_cs_table_passes", "n_cs_table_rows",
        "n_cs_forced_rounds", "n_cs_crew_passes", "n_cs_crew_jobs")


def test_the_plan_has_one_home_and_no_device_code():
    strip = lambda t: re.sub(r"//[^\n]*", "", t)
    plan = strip(open(os.path.join(CSRC, "cov_plan.hpp")).read())
    assert not re.search(r"hip|__global__|__device__|__host__|__shared__|threadIdx|blockIdx", plan, flags=re.I)
    for name in MOVED:
        assert len(re.findall(r"constexpr [\w ]*\b%s\b\s*(?:=|\()" % name, plan)) == 1, name
    for fname in sorted(os.listdir(CSRC)):
        if not fname.endswith((".hip", ".hpp", ".h")) or fname == "cov_plan.hpp":
            continue
        raw = open(os.path.join(CSRC, fname)).read()
        txt = strip(raw)
        for name in MOVED:
            assert not re.search(r"(constexpr|inline)[\w ]*\b%s\b\s*(=|\()" % name, txt), (fname, name)
        assert not re.search(r"\bcs_lds_bytes\s*\(|\bcs_ucap\s*\(", txt), fname            # nobody else computes them
        assert not re.search(r"36 \* 1024|134 \* 1024", txt), fname
        for name in GONE:
            assert not re.search(r"\b%s\b" % name, raw), (fname, name)
    solve = open(os.path.join(CSRC, "cov_solve.hpp")).read()
    assert solve.count("cs_plan(") == 1 and solve.count("cs_dev_bytes(") == 1 and solve.count("cs_pin_layout(") == 1
    assert solve.index("cs_probe_lds(cp);") < solve.index("cs_plan(in)") < solve.index("CHK(cs_alloc(h));")
    assert "static_assert(R::N <= kCsTableRec" in solve                       # kCsTableLds against GramRec<4>::N, where GramRec is visible
