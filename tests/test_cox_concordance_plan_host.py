"""What csrc/cox_plan.hpp adds for the concordance index, without a GPU: the concordance order with every event's range
(cox_conc_order) against its Python restatement (tests/_cox_concordance_numpy.py: conc_order), the level arithmetic
(cox_conc_take, cox_conc_fringe) and the group's layout (cox_conc_layout), as a stand-alone program under the host sanitizers
(tests/cox_concordance_plan_main.cpp), which also walks the whole count the way the kernels do and holds it to the pairs
counted directly."""
import os
import subprocess

import numpy as np
import pytest

import _cox_concordance_numpy as CC
import _cox_plan as CP

HERE = os.path.dirname(os.path.abspath(__file__))
T = CP.TILE


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coxc") / "cox_concordance_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cox_concordance_plan_main.cpp")], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


def test_the_levels_tile_every_range_and_the_walk_counts_the_pairs(plan_exe):
    """For every 0 <= a <= b <= 70 the runs taken over all levels tile [a, b) exactly once; the fringes and the levels from the
    tile's up do the same up to 5 T + 3; the kernels' walk equals the definition at n = 1, 2, 65, T, T + 1, 2 T + 1, 3 T - 5 and
    5 T + 3."""
    assert CC.TILE == T and 1 << CC.TILE_LOG == T
    assert "cox_concordance_plan_main OK tile=%d" % T in _run(plan_exe)


def test_the_python_walk_tiles_every_range():
    for b in range(71):
        for a in range(b + 1):
            hit = np.zeros(71, dtype=int)
            for lev in range(8):
                runs = CC.take(a, b, lev)
                assert len(runs) <= 2
                for m in runs:
                    assert a <= m << lev and (m + 1) << lev <= b
                    hit[m << lev:(m + 1) << lev] += 1
            assert np.array_equal(hit, (np.arange(71) >= a) & (np.arange(71) < b)), (a, b)
    for a, b in ((0, 0), (5, 900), (5, 1024), (5, 1025), (1023, 2049), (1024, 5123), (1025, 5123), (3000, 3100), (2047, 2049)):
        a1, b0 = CC.fringe(a, b)
        assert a <= a1 <= b0 <= b and (a1 == b0 or (a1 % T == 0 and b0 % T == 0))
        got = sorted((m << lev, (m + 1) << lev) for lev in range(CC.TILE_LOG, 14) for m in CC.take(a, b, lev))
        assert sum(hi - lo for lo, hi in got) == b0 - a1
        assert all(x[1] == y[0] for x, y in zip(got, got[1:])) and (not got or (got[0][0], got[-1][1]) == (a1, b0))


def test_layout_of_the_concordance_group(plan_exe):
    """Nine vectors of N doubles back to back, four doubles a tile and the four of the result; three vectors of N int32: a
    partition, N the padded length rounded up to whole tiles."""
    lds = (32, T, T + 32, 5 * T + 32)
    for ld, line in zip(lds, _run(plan_exe, "layout", *lds).split("\n")):
        got = [int(x) for x in line.split()]
        N = -(-ld // T) * T
        tiles = N // T
        assert got == [N, tiles] + [i * N for i in range(10)] + [9 * N + 4 * tiles, 9 * N + 4 * tiles + 4, 0, N, 2 * N, 3 * N], ld


def _order_case(exe, time, status, strata):
    n = len(time)
    ld = (n + 31) // 32 * 32
    N = -(-ld // T) * T
    g = np.zeros(n, dtype=int) if strata is None else strata
    args = [x for row in zip(time, status, g) for x in (repr(float(row[0])), int(row[1]), int(row[2]))]
    lines = _run(exe, "order", ld, N, 0 if strata is None else 1, *args).split("\n")
    got = [np.array([int(x) for x in line.split()], dtype=np.int32) for line in lines[:3]]
    want = CC.conc_order(time, status, strata, ld, N)
    for a, b, name in zip(got, want, ("corder", "qa", "qb")):
        assert np.array_equal(a, b), name
    return got


def test_the_concordance_order_and_the_ranges(plan_exe):
    # by hand: stratum 0 holds a group of events only (t = 1), a mixed group (t = 2) and a censored-only group (t = 3);
    # stratum 4 ends with a group of events only -- the group at a stratum's end AND the last row of the last stratum
    time = np.array([2.0, 1.0, 3.0, 2.0, 1.0, 2.0, 3.0, 5.0, 4.0, 5.0])
    status = np.array([0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    strata = np.array([0, 0, 0, 0, 0, 0, 0, 4, 4, 4])
    corder, qa, qb = _order_case(plan_exe, time, status, strata)
    assert list(corder[:10]) == [1, 4, 3, 5, 0, 2, 6, 8, 7, 9]
    assert list(qa[:10]) == [2, 2, 4, 4, 0, 0, 0, 0, 10, 10] and list(qb[:10]) == [7, 7, 7, 7, 0, 0, 0, 0, 10, 10]
    assert list(corder[10:32]) == list(range(10, 32)) and np.all(corder[32:] == -1)          # the pads in place, then nothing
    assert not qa[10:].any() and not qb[10:].any() and len(corder) == T
    # random, heavy ties, with and without strata; one time for all; no censoring; no strata means one range end for all
    rng = np.random.default_rng(3)
    for n, strat in ((61, True), (61, False), (97, True), (1, False), (2, False)):
        t = np.ceil(3.0 * rng.exponential(1.0, n)) / 2.0
        s = (rng.random(n) < 0.6).astype(np.float64)
        g = 7 * rng.integers(0, 3, n) - 3 if strat else None
        _, qa, qb = _order_case(plan_exe, t, s, g)
        if not strat:
            assert set(qb[qa < qb]) <= {n}
    _order_case(plan_exe, np.ones(40), (rng.random(40) < 0.5).astype(np.float64), None)
    _order_case(plan_exe, np.ceil(4 * rng.random(40)), np.ones(40), rng.integers(0, 2, 40))
