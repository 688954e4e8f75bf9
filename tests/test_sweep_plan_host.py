"""The launch plan of the streamed sweep without a GPU (csrc/sweep_plan.hpp): compiled with g++ -- through a ctypes shim against
its Python restatement (tests/_sweep_plan.py, from which the GPU tests size their shapes and name their branches), and as a
stand-alone program under the host sanitizers -- and checked by value where a number follows from arithmetic that can be
written next to it."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import _sweep_plan as SP

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "coordinatedescent.jl_amd", "csrc")
DTYPES = (np.float64, np.float32)
WIDTHS = (2, 4, 8, 16, 32, 64, "coord")
LTS, KSS, CUS = (0, 1, 2), (0, 1, 2), (1, 8, 64, 256, 304)
SIZE_FIELDS = ("ld", "nvec", "cap", "blockB", "cus", "step_grid", "block_grid", "gram_units", "partials_doubles")
OFFSETS = lambda nv: (-nv, -1, 0, 1, nv)               # a vector less, a row less, the edge, a row more (one vector more), a vector more


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sweepplan") / "libsweepplanshim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "sweep_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    i64, i32, u32, P = C.c_int64, C.c_int, C.c_uint, C.POINTER
    for name, args, res in (("sp_c_const", [C.c_char_p], i64), ("sp_c_gram_rec", [i32], i64), ("sp_c_block_rec", [i32], i64),
                            ("sp_c_sizes", [i32, i64, i64, i32, P(i64)], None),
                            ("sp_c_gram", [i64, i64, i32, i32, i32, i32, i32, P(i64)], None),
                            ("sp_c_gram_read_grid", [i64, i32], i32), ("sp_c_elementwise_grid", [i64, i64], i32),
                            ("sp_c_col_dots", [i64, i64, i32, i32, P(i64)], None),
                            ("sp_c_route", [i32, i32, i32, i32, u32, i32, P(C.c_uint64)], None),
                            ("sp_c_traffic", [i32, i32, i32, i32, P(C.c_double), i64, i64, P(i64), P(C.c_double)], None)):
        getattr(L, name).argtypes, getattr(L, name).restype = args, res
    return L


def c_sizes(shim, n, p, dtype, cus):
    out = (C.c_int64 * 9)()
    shim.sp_c_sizes(int(SP.esz(dtype) == 8), n, p, cus, out)
    return dict(zip(SIZE_FIELDS, out))


def c_gram(shim, n, dtype, B, cus, lt=2, ks=0):
    out = (C.c_int64 * 5)()
    shim.sp_c_gram(SP.nvec(n, dtype), n, cus, B // 16, SP.esz(dtype), lt, ks, out)
    return {"variant": out[0], "CVN": out[1], "nchunks": out[2], "G": out[3], "rounds": out[4]}


def twin_gram(n, dtype, B, cus, lt=2, ks=0):
    g = SP.gram_launch(n, dtype, B, cus, lt, ks)
    return {"variant": SP.VARIANT_CODE[g["variant"]], "CVN": g["CVN"], "nchunks": g["nchunks"], "G": g["G"], "rounds": g["rounds"]}


def c_col_dots(shim, bc, n, dtype, cus, width):
    out = (C.c_int64 * 3)()
    shim.sp_c_col_dots(bc, SP.nvec(n, dtype), cus, width, out)
    return tuple(out)


def c_route(shim, block_mode, B, has_w, m, xbits=0, dup=False):
    out = (C.c_uint64 * 4)()
    shim.sp_c_route(int(block_mode), B, int(has_w), m, xbits, int(dup), out)
    return bool(out[0]), bool(out[1]), int(out[2]), int(out[3])


def c_traffic(shim, blocked, B, m, has_w, hs, n, esz):
    arr, nl, nb = (C.c_double * m)(*hs), C.c_int64(), C.c_double()
    shim.sp_c_traffic(int(blocked), B, m, int(has_w), arr, n, esz, C.byref(nl), C.byref(nb))
    return nl.value, nb.value


def edges(dtype, cus):
    """Rows at which something in the plan changes, for this storage type and CU count (the same number for every pair)."""
    nv, W = SP.nv(dtype), SP.K_GRAM_WAVES
    e = [1, 32, nv, 64 * nv, 256 * nv]                                             # the ld pad, one vector, one chunk, one unit
    e += [1024 * min(SP.K_MAX_STEP_GRID, SP.K_STEP_GRID_PER_CU * cus) * nv,        # units cross the cap of the grid: k_step,
          256 * SP.K_BLOCK_GRID_PER_CU * cus * nv]                                 # k_blockstep,
    e += [256 * pc * cus * nv for pc in (2, 3)]                                    # k_gramstep sized for 64-vector chunks, per-CU 2 and 3,
    e += [cvn * W * pc * cus * nv for pc in (2, 3) for cvn in (16, 32)]            # ... and for shorter chunks
    e += [cvn * W * pc * cus * 3 * nv for pc in (2, 3) for cvn in (16, 32, 64)]    # nchunks a multiple of 4 G: a full last round
    e += [64 * SP.K_SHORT_ROUNDS * W * pc * cus * nv for pc in (2, 3)]             # rounds64 reaches kShortRounds on a full grid
    e += [SP.K_LT_LONG_ROWS, SP.K_WIDE64_ROWS, 10_000_000]
    return [max(1, x + d) for x in e for d in OFFSETS(nv)]


N_EDGES = 5 + 2 + 2 + 4 + 6 + 2 + 3


def test_constants_are_the_parents(shim):
    for name, want in (("kSpBlock", 256), ("kSpUnroll", 4), ("kSpNSum", 4), ("kSpColGroup", 8), ("kSpGramWaves", 4), ("kSpGramChunk", 64),
                       ("kStepGridPerCU", 8), ("kMaxStepGrid", 2048), ("kBlockGridPerCU", 3), ("kSpColChunks", 64), ("kSpColBatch", 4096),
                       ("kColFillPerCU", 8), ("kMaxBlockB", 8), ("kShortRounds", 16), ("kGramGridPerCU", 2), ("kGram32GridPerCU", 3),
                       ("kLtGridPerCU", 2), ("kLtLongRows", 2000000), ("kWide64Rows", 512 * 4 * 64 * 2), ("kInitGridCap", 2048),
                       ("kWeightsGridCap", 2048), ("kMomentsGridCap", 1024)):
        assert shim.sp_c_const(name.encode()) == want, name
    assert (SP.K_BLOCK, SP.K_UNROLL, SP.K_NSUM, SP.K_COL_GROUP, SP.K_GRAM_WAVES) == (256, 4, 4, 8, 4)
    assert (SP.K_COL_BATCH, SP.K_COL_CHUNKS, SP.K_WIDE64_ROWS, SP.K_LT_LONG_ROWS) == (4096, 64, 262144, 2000000)
    for NG in (1, 2, 4):
        assert shim.sp_c_gram_rec(NG) == SP.gram_rec(NG)
    assert [SP.gram_rec(NG) for NG in (1, 2, 4)] == [273, 801, 2625]                # 1, 3, 10 tiles of 256, then B dots and r'r
    for B in (2, 4, 8):
        assert shim.sp_c_block_rec(B) == SP.block_rec(B)
    # the kernels' own constants and record sizes are tied to these where both are visible
    hip = open(os.path.join(CSRC, "cdhip.hip")).read()
    assert "kSpBlock == kBlock && kSpUnroll == kUnroll && kSpNSum == kNSum && kSpColGroup == kColGroup && kSpGramWaves == kGramWaves" in hip
    assert "static_assert(kSpColBatch == kColBatch && kSpColChunks == kColChunks" in hip   # the batch loop's two sizes, by their own names
    assert "sp_gram_rec(4) == GramRec<4>::N" in hip and "sp_block_rec(kMaxBlockB) == BlockRec<kMaxBlockB>::N" in hip


def test_plan_is_the_twins_over_the_cross_product(shim):
    wide = narrow = 0
    for dtype, cus in itertools.product(DTYPES, CUS):
        ns = edges(dtype, cus)
        assert len(ns) == 5 * N_EDGES
        for n in ns:
            sizes = c_sizes(shim, n, 70, dtype, cus)
            assert sizes == SP.sweep_sizes(n, 70, dtype, cus), (dtype, cus, n)
            assert shim.sp_c_elementwise_grid(sizes["nvec"], 2048) == SP.init_grid(n, dtype)
            assert shim.sp_c_elementwise_grid(sizes["nvec"], 1024) == SP.elementwise_grid(n, dtype, SP.K_MOMENTS_GRID_CAP)
            assert shim.sp_c_gram_read_grid(sizes["nvec"], cus) == SP.gram_grid(n, dtype, cus)[0]
            for bc, width in itertools.product((1, 8, 9, 70, 4095, 4096), (1, 2)):
                assert c_col_dots(shim, bc, n, dtype, cus, width) == SP.col_dots_plan(bc, n, dtype, cus, width)
            # the knobs reach the wide-block launch only: its plan over width x CDH_LT x CDH_KS ...
            for B, lt, ks in itertools.product((16, 32, 64), LTS, KSS):
                got, want = c_gram(shim, n, dtype, B, cus, lt, ks), twin_gram(n, dtype, B, cus, lt, ks)
                assert got == want, (dtype, cus, n, B, lt, ks, got, want)
                wide += 1
            # ... and once per narrow width and for the per-coordinate sweep (fixed grids, compared above): the route of a chunk
            for B in (2, 4, 8, "coord"):
                mode, Bn = B != "coord", (32 if B == "coord" else B)
                for has_w, m in itertools.product((False, True), (1, 7, 8, 2 * Bn - 1, 2 * Bn, 70)):
                    assert c_route(shim, mode, Bn, has_w, m) == SP.chunk_route(mode, Bn, has_w, m)
                narrow += 1
    # distinct comparisons, not the 7 x 3 x 3 product: a narrow width has no knob to vary
    assert wide == 2 * 5 * 5 * N_EDGES * 3 * 3 * 3 == 32400 and narrow == 2 * 5 * 5 * N_EDGES * 4 == 4800
    assert set(WIDTHS) == {16, 32, 64, 2, 4, 8, "coord"}


def test_sizes_by_value(shim):
    s = c_sizes(shim, 3000, 5000, np.float64, 256)
    assert (s["ld"], s["nvec"], s["cap"], s["blockB"]) == (3008, 1500, 5000, 64)
    assert (s["step_grid"], s["block_grid"], s["gram_units"]) == (2, 6, 6) == (-(-1500 // 1024), -(-1500 // 256), -(-1500 // 256))
    assert [c_sizes(shim, n, 1, np.float64, 256)["ld"] for n in (1, 31, 32, 33)] == [32, 32, 32, 64]
    assert [c_sizes(shim, n, 1, np.float32, 256)["nvec"] for n in (1, 4, 5)] == [1, 1, 2]
    assert c_sizes(shim, 10, 1, np.float64, 8)["cap"] == 4096
    # the default width: 64 on fp64 columns short of 512 blocks x 4 waves x 64 vectors x 2 rows, 32 otherwise
    assert [c_sizes(shim, n, 1, np.float64, 256)["blockB"] for n in (262143, 262144)] == [64, 32] and 512 * 4 * 64 * 2 == 262144
    assert [c_sizes(shim, n, 1, np.float32, 256)["blockB"] for n in (3000, 262143, 262144)] == [32, 32, 32]
    # the step grid: 8 per CU until 256 CUs, 2048 beyond
    big = 10_000_000
    assert [c_sizes(shim, big, 1, np.float64, c)["step_grid"] for c in (1, 8, 255, 256, 304)] == [8, 64, 2040, 2048, 2048]
    assert [c_sizes(shim, big, 1, np.float64, c)["block_grid"] for c in (1, 256, 304)] == [3, 768, 912]
    # the partials: the column dots' 4096 x 64 pairs until the B = 64 records of 2 blocks per CU outgrow them
    assert c_sizes(shim, big, 1, np.float64, 8)["partials_doubles"] == 4096 * 64 * 2 == 524288
    assert 2 * 99 * 2625 < 524288 < 2 * 100 * 2625 and 3 * 304 * 801 < 2 * 304 * 2625
    assert [c_sizes(shim, big, 1, np.float64, c)["partials_doubles"] for c in (99, 100, 304)] == [524288, 525000, 2 * 304 * 2625]


def test_no_refusal_is_reachable(shim):
    """Every record set a launch writes fits what cdh_create allocated: the bounds in the launchers never fire."""
    for dtype, cus in itertools.product(DTYPES, CUS):
        for n in edges(dtype, cus):
            s = c_sizes(shim, n, 70, dtype, cus)
            room = s["partials_doubles"]
            assert s["step_grid"] * SP.K_NSUM <= room and s["block_grid"] * SP.block_rec(8) <= room
            assert SP.elementwise_grid(n, dtype, SP.K_MOMENTS_GRID_CAP) * SP.K_NSUM <= room               # k_resid_moments
            assert shim.sp_c_gram_read_grid(s["nvec"], cus) * SP.gram_rec(4) <= room                          # cdh_gram
            for B, lt, ks in itertools.product((16, 32, 64), LTS, KSS):
                assert c_gram(shim, n, dtype, B, cus, lt, ks)["G"] * SP.gram_rec(B // 16) <= room
            for bc in (1, 9, 4095, SP.K_COL_BATCH):
                groups, chunks, doubles = c_col_dots(shim, bc, n, dtype, cus, 2)
                assert doubles == groups * chunks * 16 <= room and c_col_dots(shim, bc, n, dtype, cus, 1)[2] == groups * chunks * 8
                # vc_point: expanded columns of a batch in whole base groups of Q + 1 (one group more than the batch at most), each
                # `chunks` sums, twice with a left-out row
                for Q1 in (2, 3, 4):
                    assert (-(-bc // Q1) + 1) * Q1 * chunks * 2 <= room
    assert 4096 * 64 * 2 >= 1024 * 6                                                 # the IRLS records: kGlmMaxGrid x kGlmPoisVals
    assert "kColBatch * kColChunks * 2 >= (size_t)kGlmMaxGrid * kGlmPoisVals" in open(os.path.join(CSRC, "cdhip.hip")).read()


def test_every_chunk_is_handed_out_exactly_once(shim):
    """k_gramstep's loop replayed -- `for (ch = wave * G + block; ch < nchunks; ch += 4 * G)` for every wave of every block -- over
    the plan's grid and chunk count, at every edge, a row below it and a row above it, for every width and knob.  The loop sees
    (G, nchunks) only, so each distinct pair is replayed once."""
    replayed = set()
    for dtype, cus in itertools.product(DTYPES, CUS):
        ns = edges(dtype, cus)
        for n in ns[1::5] + ns[2::5] + ns[3::5]:
            for B, lt, ks in itertools.product((16, 32, 64), LTS, KSS):
                g = c_gram(shim, n, dtype, B, cus, lt, ks)
                nvec, G, nch = SP.nvec(n, dtype), g["G"], g["nchunks"]
                assert g["CVN"] * nch >= nvec > g["CVN"] * (nch - 1)
                if (G, nch) in replayed:
                    continue
                replayed.add((G, nch))
                stride, trips = 4 * G, -(-nch // (4 * G))
                first = (np.arange(4)[:, None] * G + np.arange(G)[None, :]).ravel()              # ch = wave * G + block
                ch = first[:, None] + stride * np.arange(trips)[None, :]                          # ch += 4 * G, `trips` times at most
                ran = ch < nch                                                                    # ... while ch < nchunks
                assert np.array_equal(np.bincount(ch[ran], minlength=nch), np.ones(nch, dtype=np.int64)), (dtype, cus, n, B, lt, ks)
                assert int(ran.sum(axis=1).max()) == g["rounds"]                                  # the most trips any wave makes
    # what was replayed: launches of one round with idle waves and with none, of several rounds with a full last one and a ragged one
    kinds = {(nch <= 4 * G, nch % (4 * G) == 0) for G, nch in replayed}
    assert kinds == {(True, False), (True, True), (False, True), (False, False)}, kinds


def test_variant_table(shim):
    """The default knobs: fragment loads only for B = 16 below 2e6 rows and for fp32 B = 64; short chunks below 16 rounds."""
    F, L, S = (SP.VARIANT_CODE[k] for k in (SP.FRAG, SP.LT_LONG, SP.LT_SHORT))
    for cus in CUS:
        for n in (1, 3000, 262144, 1_999_999, 2_000_000, 10_000_000):
            long16 = n >= 2_000_000
            for dtype in DTYPES:
                got = {B: c_gram(shim, n, dtype, B, cus)["variant"] for B in (16, 32, 64)}
                assert got[16] == (L if long16 else F), (cus, n)
                assert got[32] in (L, S)
                assert got[64] == F if dtype == np.float32 else got[64] in (L, S)
                # knobs: CDH_LT=0 is the fragment path everywhere; CDH_LT=1 with CDH_KS pins the chunk length; B = 16 stays long
                assert {c_gram(shim, n, dtype, B, cus, lt=0, ks=ks)["variant"] for B in (16, 32, 64) for ks in KSS} == {F}
                assert c_gram(shim, n, dtype, 32, cus, lt=1, ks=1)["variant"] == S and c_gram(shim, n, dtype, 32, cus, lt=1, ks=2)["variant"] == L
                assert {c_gram(shim, n, dtype, 16, cus, lt=1, ks=ks)["variant"] for ks in KSS} == {L}
                assert {c_gram(shim, n, dtype, 64, cus, lt=lt, ks=ks)["variant"] for lt in LTS for ks in KSS} == ({F} if dtype == np.float32 else {F, L, S})
    # the cut by value, 256 CUs, B = 32 (2 per CU: 512 blocks of 4 waves): rounds64 = floor(ceil(nvec / 64) / 2048) reaches 16 at nvec = 64 * 32768
    edge = 64 * 16 * 2048
    assert [c_gram(shim, 2 * nvec, np.float64, 32, 256)["variant"] for nvec in (edge - 64, edge - 63, edge)] == [S, L, L]
    g = c_gram(shim, 3000, np.float64, 64, 256)                  # the short column of the comments: 94 chunks of 16 vectors on 24 blocks
    assert (g["variant"], g["CVN"], g["nchunks"], g["G"], g["rounds"]) == (S, 16, 94, 24, 1)


def _transcribed_traffic(blocked, B, m, has_w, h_hs, n, esz, prof_launches=0, prof_bytes=0.0):
    """run_chunk's profile block as it stood in cdhip.hip before the plan existed, statement by statement, adding to the handle's
    running totals."""
    vec = float(n) * float(esz)
    if not blocked:
        prof_launches += m
        for i in range(m):
            ap = i > 0 and h_hs[i - 1] != 0.0
            prof_bytes += vec * ((3.0 if has_w else 2.0) + (2.0 if ap else 0.0))
        if h_hs[m - 1] != 0.0:
            prof_bytes += 3.0 * vec
    else:
        pos0 = 0
        while pos0 < m:
            nb = min(B, m - pos0)
            nzp = 0
            for i in range(max(0, pos0 - B), pos0):
                nzp += h_hs[i] != 0.0
            prof_bytes += vec * (nb + 1 + nzp + (1 if nzp else 0))
            prof_launches += 1
            pos0 += B
        nzl = 0
        for i in range(((m - 1) // B) * B, m):
            nzl += h_hs[i] != 0.0
        if nzl:
            prof_bytes += vec * (nzl + 2)
    return prof_launches, prof_bytes


def _move_patterns(m, B):
    last_of_block = [float((i + 1) % B == 0 or i == m - 1) for i in range(m)]
    return {"none": [0.0] * m, "all": [0.25] * m, "last_visit": [0.0] * (m - 1) + [-1.5], "last_of_a_block": last_of_block,
            "first_of_a_block": [float(i % B == 0) for i in range(m)]}


def test_chunk_traffic_is_the_parents_model(shim):
    count = 0
    for B in (1, 2, 4, 8, 16, 32, 64):
        blocked = B > 1
        for m in sorted({1, max(1, B - 1), B, B + 1, 2 * B + 6}):
            for name, hs in _move_patterns(m, max(B, 2)).items():
                for has_w, (n, esz) in itertools.product((False, True), ((1000, 8), (1000, 4), (10_000_019, 8), (999_999, 4))):
                    want = _transcribed_traffic(blocked, B, m, has_w, hs, n, esz)
                    assert c_traffic(shim, blocked, B, m, has_w, hs, n, esz) == want, (B, m, name, has_w, n, esz)
                    assert SP.chunk_traffic(blocked, B, m, has_w, [h != 0.0 for h in hs], n, esz) == want
                    count += 1
    assert count == (3 + 4 + 5 * 5) * 5 * 2 * 4                  # distinct m: {1, 2, 8} per coordinate, {1, 2, 3, 10} at B = 2, five from B = 4 on
    # a bracket of several chunks: the plan sums each chunk from zero and the caller adds the sums, where every term once went
    # into the running total one by one.  Every term is an integer number of bytes, so below 2^53 the grouping cannot show.
    total_l, total_b, run_l, run_b = 0, 0.0, 0, 0.0
    for B, m in ((64, 134), (32, 70), (1, 9), (64, 63)) * 50:
        hs = _move_patterns(m, max(B, 2))["first_of_a_block"]
        nl, nb = c_traffic(shim, B > 1, B, m, True, hs, 10_000_019, 8)
        assert nb == int(nb) and nb < 2.0 ** 53
        total_l, total_b = total_l + nl, total_b + nb
        one_l, one_b = _transcribed_traffic(B > 1, B, m, True, hs, 10_000_019, 8, run_l, run_b)
        run_l, run_b = one_l, one_b
    assert (total_l, total_b) == (run_l, run_b) and total_b < 2.0 ** 53
    # by value: a per-coordinate chunk of 3 visits that all move reads (x, r) three times, rewrites r twice in the next visit's
    # launch (read x, write r: 2 more) and once in the trailing axpy (read x, read r, write r)
    assert c_traffic(shim, False, 1, 3, False, [1.0, 1.0, 1.0], 1000, 8) == (3, 8000.0 * (2 + 4 + 4 + 3))
    # a blocked chunk of B + 1 visits, all moving: launch 1 reads B columns and r; launch 2 reads 1 column and r, re-reads the B
    # columns that moved and writes r; the trailing axpy reads 1 column and r and writes r
    assert c_traffic(shim, True, 16, 17, False, [1.0] * 17, 1000, 8) == (2, 8000.0 * ((16 + 1) + (1 + 1 + 16 + 1) + (1 + 2)))


def test_chunk_route_and_graph_key(shim):
    # blocked: block mode, and with observation weights only the wide-block kernel (B >= 16)
    for mode, B, has_w in itertools.product((False, True), (2, 4, 8, 16, 32, 64), (False, True)):
        blocked = c_route(shim, mode, B, has_w, 100)[0]
        assert blocked == (mode and (not has_w or B >= 16))
        for m in (1, 7, 8, 2 * B - 1, 2 * B, 2 * B + 1, 4096):
            got = c_route(shim, mode, B, has_w, m)
            assert got == SP.chunk_route(mode, B, has_w, m)
            assert got[1] == (m >= (2 * B if blocked else 8))                       # a graph of one or two launches saves nothing
            assert got[3] == ((-(-m // B) + 1) if blocked else m + 1)               # launches that rewrite r
    # the key: m above bit 20, the width (0: per coordinate) at bits 8 .. 14, the exchange's bits 16 | 32, dup 4, weights 2
    xs = open(os.path.join(CSRC, "exchange_state.hpp")).read()
    assert "graph_key_bits() const { return (comm_ ? 32u : 0u) | (p2p_on_ ? 16u : 0u); }" in xs
    XBITS = (0, 16, 32, 48)
    assert all(x & (2 | 4) == 0 and x < (1 << 8) for x in XBITS) and (64 << 8) < (1 << 20)
    seen = {}
    for mode, B, has_w, dup, xbits, m in itertools.product((False, True), (2, 4, 8, 16, 32, 64), (False, True), (False, True), XBITS,
                                                            (8, 9, 64, 70, 128, 4095, 4096, 100003)):
        blocked, _, key, _ = c_route(shim, mode, B, has_w, m, xbits, dup)
        assert key == (m << 20) | ((B if blocked else 0) << 8) | xbits | (4 if dup else 0) | (2 if has_w else 0)
        what = (m, blocked, B if blocked else 0, xbits, dup, has_w)                 # what the launch sequence depends on
        assert seen.setdefault(key, what) == what
    assert len(seen) == len(set(seen.values()))


@pytest.mark.parametrize("fault", ["lt_per_cu_3", "short_cut_le", "grid_of_64_chunks"])
def test_a_planted_error_fails_the_comparison(shim, monkeypatch, fault):
    """The cross product is fine enough to tell the header from a twin with one rule wrong."""
    def mismatches():
        return sum(c_gram(shim, n, dtype, B, cus, lt, ks) != twin_gram(n, dtype, B, cus, lt, ks)
                   for dtype, cus in itertools.product(DTYPES, CUS) for n in edges(dtype, cus)
                   for B, lt, ks in itertools.product((16, 32, 64), LTS, KSS))
    assert mismatches() == 0
    monkeypatch.setattr(SP, "FAULT", fault)
    assert mismatches() > 0


def test_sanitized_stand_alone_program(tmp_path):
    exe = str(tmp_path / "sweep_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "sweep_plan_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "sweep_plan_main OK" in out


MOVED = ("kStepGridPerCU", "kMaxStepGrid", "kBlockGridPerCU", "kMaxBlockB", "kShortRounds", "kGramGridPerCU",
         "kGram32GridPerCU", "kLtGridPerCU", "balanced_grid", "gram_blocks_per_cu", "elementwise_grid", "gram_plan", "col_dots_plan",
         "chunk_route", "chunk_traffic", "sweep_sizes", "gram_read_grid")


def test_the_plan_has_one_home_and_no_device_code():
    strip = lambda t: re.sub(r"//[^\n]*", "", t)
    plan = strip(open(os.path.join(CSRC, "sweep_plan.hpp")).read())
    assert not re.search(r"hip|__global__|__device__|__host__|__shared__|threadIdx|blockIdx|#include\s*\"", plan, flags=re.I)
    for name in MOVED:
        assert len(re.findall(r"constexpr [\w ]*\b%s\b\s*(?:=|\()" % name, plan)) == 1, name
    for fname in sorted(os.listdir(CSRC)):
        if not fname.endswith((".hip", ".hpp", ".h")) or fname == "sweep_plan.hpp":
            continue
        txt = strip(open(os.path.join(CSRC, fname)).read())
        for name in MOVED:
            assert not re.search(r"(constexpr|inline)[\w ]*\b%s\b\s*(=|\()" % name, txt), (fname, name)
        # nobody else sizes a grid from the CU count or caps an elementwise grid by hand
        assert not re.search(r"std::min<int64_t>\((2048|1024), \(h->nvec", txt), fname
        for gone in ("NGgrid", "col_dots_chunks", "h->step_grid", "h->block_grid", "h->gram_units", "h->partials_doubles", "prof_ms",
                     "prof_bytes", "prof_launches", "h->ev0", "h->ev1"):
            assert gone not in txt, (fname, gone)
    sweep = open(os.path.join(CSRC, "sweep.hpp")).read()
    assert sweep.count("gram_plan(") == 1 and sweep.count("chunk_route(") == 1 and sweep.count("chunk_traffic(") == 1
    dots = open(os.path.join(CSRC, "col_dots.hpp")).read()
    assert dots.count("col_dots_plan(") == 2 and dots.count("elementwise_grid(") == 1 and "getenv" not in sweep + dots
    assert dots.count('"partials too small"') == 1 and sweep.count("need_partials(") == 1          # the bound is written once
    assert sweep.index("if (h->prof.on) {") < sweep.index("chunk_traffic(")           # the model's loop runs only while profiling
    hip = open(os.path.join(CSRC, "cdhip.hip")).read()
    assert hip.count('#include "sweep.hpp"') == 1 and hip.count("sweep_sizes(") == 1
    # each include stands where its code stood: the order in which kernel templates are first used is the order of the code object
    assert hip.index("int32_t sync_r(cdh_handle h) {") < hip.index('#include "col_dots.hpp"') < hip.index("int32_t rebuild_residual_from(cdh_handle h, const cdh::SupportList& x, bool with_beta) {")
    assert hip.index("int32_t rebuild_residual(cdh_handle h)") < hip.index('#include "sweep.hpp"') < hip.index('#include "grad_cache.hpp"')
    # the profile bracket is written once
    every = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp")))
    assert every.count("hipEventElapsedTime(") == 2                                # Profile::end, and cdh_exchange_latency's own probe
    assert every.count("prof.begin(") == every.count("prof.end(") == 3 and every.count("prof.stop(") == 4
