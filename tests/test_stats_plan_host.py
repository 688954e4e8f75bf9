"""The launch plans of the statistics exports without a GPU (csrc/stats_plan.hpp: the launches and the scatter of a Gram block,
the batches of a varying-coefficient point): compiled with g++ -- through a ctypes shim against the Python restatement of the
host code these plans were taken out of (tests/_stats_plan.py), and as a stand-alone program under the host sanitizers -- and
checked by value where a number follows from arithmetic that can be written next to it."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import _stats_plan as TP
import _sweep_plan as SP

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "coordinatedescent.jl_amd", "csrc")
DTYPES = (np.float64, np.float32)
CUS = (1, 8, 64, 256, 304)
GRAM_EDGES = (1, 32, 33, 63, 64, 65, 95, 96, 97, 128, 129, 4065, 4095, 4096)
VC_ROWS = (1, 33, 513, 5003, 300_000)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("statsplan") / "libstatsplanshim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "stats_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    i64, i32, f64, P = C.c_int64, C.c_int, C.c_double, C.POINTER
    for name, args, res in (("st_c_const", [C.c_char_p], i64), ("st_c_rec_g", [i32, i32], i32), ("st_c_gram_launches", [i64], i64),
                            ("st_c_gram_launch", [i64, i64, P(i64)], i32), ("st_c_gram_groups", [i64, P(i64)], None),
                            ("st_c_gram_scatter", [i64, i64, P(f64), P(f64), P(f64), P(f64)], None),
                            ("st_c_vc_batches", [i64], i64), ("st_c_vc_batch", [i64, i32, i64, i32, i32, i64, P(i64)], None),
                            ("st_c_vc_launches", [i64, i32], i64), ("st_c_vc_bytes", [i64, i64, i64], f64),
                            ("st_c_partials_doubles", [i32, i64, i64, i32], i64)):
        getattr(L, name).argtypes, getattr(L, name).restype = args, res
    return L


def c_gram_launches(shim, m):
    out, buf = [], (C.c_int64 * 64)()
    for t in range(shim.st_c_gram_launches(m)):
        out.append(list(buf[:shim.st_c_gram_launch(m, t, buf)]))
    return out


def c_gram_groups(shim, m):
    out = np.zeros((shim.st_c_gram_launches(m), 4), dtype=np.int64)
    shim.st_c_gram_groups(m, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return out


def c_vc_plan(shim, p, degree, n, dtype, cus, loo):
    out, batches = (C.c_int64 * 7)(), []
    for t in range(shim.st_c_vc_batches(p) if degree > 0 else 0):
        shim.st_c_vc_batch(p, degree, SP.nvec(n, dtype), cus, int(loo), t, out)
        batches.append(tuple(out))
    return batches, shim.st_c_vc_launches(p, degree), shim.st_c_vc_bytes(n, SP.esz(dtype), p)


def vc_ps(degree):
    """Around every multiple of 4096 up to 3 x 4096: from 4096 k - (degree + 1) to 4096 k + (degree + 1) in steps of degree + 1,
    each rounded down to whole groups of degree + 1 columns (a design has no others)."""
    Q1 = degree + 1
    return sorted({(4096 * k + d) // Q1 * Q1 for k in (1, 2, 3) for d in (-Q1, 0, Q1)})


def test_constants_and_the_record_are_the_kernels(shim):
    for name, want in (("kGramMaxCols", 4096), ("kGramGroupCols", 32), ("kGramLaunchCols", 64), ("kGsOffC", 2560), ("kGsOffQ", 2624),
                       ("kGsRec", SP.gram_rec(4))):
        assert shim.st_c_const(name.encode()) == want, name
    assert (TP.OFF_C, TP.OFF_Q, TP.REC) == (2560, 2624, 2625)
    offs = [shim.st_c_rec_g(s, l) for s in range(64) for l in range(s, 64)]
    assert offs == [TP.rec_g(s, l) for s in range(64) for l in range(s, 64)]
    assert sorted(offs) == sorted(t * 256 + r * 16 + c for t, (gs, gl) in enumerate((a, b) for a in range(4) for b in range(a, 4))
                                  for r in range(16) for c in range(16) if gs < gl or r <= c)       # each entry of the upper triangle once
    hip = open(os.path.join(CSRC, "cdhip.hip")).read()
    assert "gs_g(s, l) != GramRec<4>::g(s, l)" in hip and "kGsOffC == GramRec<4>::OFF_C && kGsOffQ == GramRec<4>::OFF_Q && kGsRec == GramRec<4>::N" in hip
    assert 'static_assert(gram_rec_restated(), "stats_plan.hpp restates GramRec<4>");' in hip


def test_gram_launches_for_every_m(shim):
    for m in range(1, 4097):
        got = c_gram_groups(shim, m)
        ng = -(-m // 32)
        assert len(got) == (1 if m <= 64 else ng * (ng - 1) // 2), m
        a0, na, b0, nb = got.T
        # 1 .. 64 columns, distinct (two ascending runs, the second behind the first) and inside the list
        assert np.all((na >= 1) & (nb >= 0) & (na + nb <= 64) & (a0 >= 0) & (a0 + na <= b0) & (b0 + nb <= m)), m
        assert np.array_equal(got, TP.gram_launch_groups(m)), m                # the parent's launches in the parent's order
    for m in GRAM_EDGES[:-3] + (200,):                                        # ... and column by column, position by position
        assert c_gram_launches(shim, m) == TP.gram_launches(m), m
    assert c_gram_launches(shim, 65) == [list(range(64)), list(range(32)) + [64], list(range(32, 64)) + [64]]
    assert c_gram_launches(shim, 4096)[-1] == list(range(4032, 4096)) and c_gram_launches(shim, 4065)[-1] == list(range(4032, 4064)) + [4064]


@pytest.mark.parametrize("m", GRAM_EDGES)
def test_gram_scatter_is_the_parents_two_loops(shim, m):
    """Launch t's record says, entry by entry, which pair of columns it stands for: G[s][l] -> t + (col_s * 4096 + col_l) / 2^24,
    c[pos] -> -(t + col / 4096), q -> 1000 + t.  The header's one scatter and the twin's two loops then leave the same arrays --
    the same launch's value where several hold an entry -- and no entry is left unwritten."""
    launches = TP.gram_launches(m)
    records = []
    for t, cols in enumerate(launches):
        rec, k, col = np.full(TP.REC, np.nan), len(cols), np.array(cols)
        ps, pl = np.triu_indices(k)                                              # positions s <= l: the columns ascend with them
        rec[TP.REC_G[ps, pl]] = t + (col[ps] * 4096 + col[pl]) / 2.0 ** 24
        rec[TP.OFF_C:TP.OFF_C + k] = -(t + col / 4096.0)
        rec[TP.OFF_Q] = 1000 + t
        records.append(rec)
    want_G, want_c, want_q = TP.gram_scatter(m, records)
    G, c, q = np.full((m, m), np.nan), np.full(m, np.nan), C.c_double(np.nan)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for t, rec in enumerate(records):
        shim.st_c_gram_scatter(m, t, pd(rec), pd(G), pd(c), C.byref(q))
    assert not np.isnan(G).any() and not np.isnan(c).any()                     # every out_G[i, j] and every out_c[i] is written
    assert np.array_equal(G, want_G) and np.array_equal(c, want_c) and q.value == want_q == 1000 + len(launches) - 1
    # what an entry holds is its pair of columns, smaller first, whichever launch wrote it last
    i, j = np.indices((m, m))
    assert np.array_equal(G - np.floor(G), (np.minimum(i, j) * 4096 + np.maximum(i, j)) / 2.0 ** 24)
    # without out_c and out_q nothing but G is touched
    G2 = np.full((m, m), np.nan)
    for t, rec in enumerate(records):
        shim.st_c_gram_scatter(m, t, pd(rec), pd(G2), None, None)
    assert np.array_equal(G2, G)


def test_vc_plan_over_the_grid(shim):
    straddles, compared = set(), 0
    for degree, loo, cus, dtype, n in itertools.product((1, 2, 3), (False, True), CUS, DTYPES, VC_ROWS):
        Q1 = degree + 1
        room = shim.st_c_partials_doubles(int(SP.esz(dtype) == 8), n, 4096, cus)
        assert room == SP.sweep_sizes(n, 4096, dtype, cus)["partials_doubles"]
        for p in vc_ps(degree):
            batches, launches, nbytes = c_vc_plan(shim, p, degree, n, dtype, cus, loo)
            want = TP.vc_point_plan(p, degree, n, dtype, cus, loo)
            assert (batches, launches) == want[:2], (degree, loo, cus, n, p)
            assert nbytes == want[2] == float(n) * float(SP.esz(dtype)) * (float(p) + 2.0)     # the parent's expression, bit for bit
            compared += 1
            # the batches tile [0, p)
            assert [b[0] for b in batches] == list(range(0, p, 4096)) and [b[1] for b in batches] == [min(b0 + 4096, p) for b0 in range(0, p, 4096)]
            held = np.zeros(p // Q1, dtype=np.int64)                      # in how many batches a base column is
            for t, (b0, b1, jb0, jb1, chunks, table, partials) in enumerate(batches):
                # [jb0, jb1) is exactly the set of base columns with an expanded column in the batch
                assert np.array_equal(np.arange(jb0, jb1), np.unique(np.arange(b0, b1) // Q1))
                assert chunks == SP.col_dots_plan(b1 - b0, n, dtype, cus, 1)[1]
                assert table == (jb1 - jb0) * Q1 * chunks and partials == table * (2 if loo else 1)
                # the refusal of need_partials is unreachable: a full batch has 512 column groups, so col_dots_plan asks for
                # ceil(8 cus / 512) <= 5 row chunks, and a batch short enough for 64 chunks has at most 8 ceil(8 cus / 64) columns
                assert partials <= room, (degree, loo, cus, n, p, partials, room)
                held[jb0:jb1] += 1
            # a base column is in two batches (neighbours: the batches ascend) iff its group straddles a batch boundary
            first = np.arange(p // Q1) * Q1
            straddle = first // 4096 != (first + degree) // 4096
            assert np.array_equal(held, 1 + straddle), (degree, p)
            straddles.update((degree, p, int(jb)) for jb in np.flatnonzero(straddle))
    assert compared == 2 * 5 * 2 * 5 * sum(len(vc_ps(d)) for d in (1, 2, 3)) == 100 * 27
    # 4096 is a multiple of 2 and of 4, not of 3: only degree 2 ever straddles, from p = 4098 on
    assert {d for d, _, _ in straddles} == {2} and min(p for _, p, _ in straddles) == 4098
    assert (2, 4098, 1365) in straddles and (2, 4095, 1364) not in straddles and (2, 4096 * 3 + 3, 2730) in straddles


def test_vc_plan_by_value(shim):
    # p = 4098 at degree 2, 256 CUs, n = 5003 in fp64 (2502 vectors: 10 blocks of rows): the full batch gets ceil(2048 / 512) = 4
    # row chunks, the batch of two columns min(64, 2048, 10) = 10; the last group, base column 1365, is in both
    batches, launches, nbytes = c_vc_plan(shim, 4098, 2, 5003, np.float64, 256, True)
    assert batches == [(0, 4096, 0, 1366, 4, 1366 * 3 * 4, 2 * 1366 * 3 * 4), (4096, 4098, 1365, 1366, 10, 30, 60)]
    assert launches == 3 and nbytes == 5003 * 8 * 4100.0
    # degree 1: the boundary falls between base columns 2047 and 2048
    assert [b[2:4] for b in c_vc_plan(shim, 4098, 1, 33, np.float32, 256, False)[0]] == [(0, 2048), (2048, 2049)]
    # degree 0 expands nothing: one launch (k_vc_weights), the scales are col_dots'
    assert c_vc_plan(shim, 4098, 0, 33, np.float64, 256, False)[:2] == ([], 1)


@pytest.mark.parametrize("fault", ["pairs_b_outer", "one_launch_le_65", "jb1_floor"])
def test_a_planted_error_fails_the_comparison(shim, monkeypatch, fault):
    """The comparisons are fine enough to tell the header from a twin with one rule wrong."""
    def mismatches():
        gram = sum(c_gram_launches(shim, m) != TP.gram_launches(m) for m in GRAM_EDGES)
        vc = sum(c_vc_plan(shim, p, degree, 5003, np.float64, 256, True)[:2] != TP.vc_point_plan(p, degree, 5003, np.float64, 256, True)[:2]
                 for degree in (1, 2, 3) for p in vc_ps(degree))
        return gram + vc
    assert mismatches() == 0
    monkeypatch.setattr(TP, "FAULT", fault)
    assert mismatches() > 0


def test_sanitized_stand_alone_program(tmp_path):
    exe = str(tmp_path / "stats_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "stats_plan_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "stats_plan_main OK" in out


def test_the_plans_and_the_read_backs_have_one_home():
    strip = lambda t: re.sub(r"//[^\n]*", "", t)
    plan = strip(open(os.path.join(CSRC, "stats_plan.hpp")).read())
    assert not re.search(r"hip|__global__|__device__|__host__|__shared__|threadIdx|blockIdx", plan, flags=re.I)
    assert re.findall(r"#include\s*\"([^\"]+)\"", plan) == ["sweep_plan.hpp"]
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".h"))}
    every = "".join(src.values())
    # the residual's sums and the column pairs come back through col_dots.hpp's helpers, and nobody else picks a pair apart
    assert every.count("h->d_red, sizeof(double) * 4") == 1 and "h->d_red, sizeof(double) * 4" in src["col_dots.hpp"]
    assert "return v[2 * j]; }" in src["col_dots.hpp"] and "return v[2 * j + 1]; }" in src["col_dots.hpp"]
    for f in ("cdhip.hip", "col_stats.hpp", "vc_host.hpp", "grad_cache.hpp", "sweep.hpp", "cv_path.hpp"):     # host code throughout
        assert not re.search(r"\[(\(size_t\)\()?2 \* \w+( \+ 1)?\)?\]", strip(src[f])), f
    assert every.count('"coordinate out of range"') == 2 and src["col_dots.hpp"].count('"coordinate out of range"') == 2
    assert every.count('"idx1: coordinate out of range"') == 1                           # cv_path.hpp's own message
    for name in ("kGramMaxCols", "gram_launches", "gram_launch_at", "gram_scatter", "vc_batch", "vc_point_launches", "vc_point_bytes"):
        assert len(re.findall(r"constexpr [\w ]*\b%s\b\s*(?:=|\()" % name, plan)) == 1, name
        assert all(not re.search(r"constexpr [\w ]*\b%s\b\s*(?:=|\()" % name, strip(t)) for f, t in src.items() if f != "stats_plan.hpp"), name
    stats, vc = src["col_stats.hpp"], src["vc_host.hpp"]
    assert stats.count("gram_launch_at(") == 1 and stats.count("gram_scatter(") == 1 and stats.count("R::g(") == 0
    assert vc.count("vc_batch(") == 1 and vc.count("vc_point_launches(") == 1 and vc.count("vc_point_bytes(") == 1 and "kColBatch" not in vc
    assert vc.count("k_vc_expand<T, 1,") == 1                                           # the kernel choice is written once
    # each include stands where its code stood: the order in which kernel templates are first used is the order of the code object
    hip = src["cdhip.hip"]
    assert hip.index("int32_t cdh_glm_poisson_irls(") < hip.index('#include "vc_host.hpp"') < hip.index("int32_t cdh_vc_gram(") < hip.index('#include "col_stats.hpp"')
    assert hip.count('#include "vc_host.hpp"') == hip.count('#include "col_stats.hpp"') == 1
