"""What csrc/cox_plan.hpp adds for cdh_glm_cox_score, without a GPU: the score group's layout (cox_score_layout), the pair tiles
of the information matrix and the regrowth, as a stand-alone program under the host sanitizers (tests/cox_score_plan_main.cpp)
and against a Python restatement of the layout."""
import os
import subprocess

import pytest

import _cox_plan as CP

HERE = os.path.dirname(os.path.abspath(__file__))
T = CP.TILE
G = CP.MAX_GRID
PAIR, MAXCOLS = 4, 64
CASES = [(32, 1), (T, 3), (T + 32, 5), (5 * T + 32, 64), (2000000, 8)]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coxs") / "cox_score_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cox_score_plan_main.cpp")], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


def test_layouts_pair_tiles_walk_and_regrowth(plan_exe):
    """Every offset disjoint from its neighbours, every pair (c, d), c <= d < m, in exactly one tile for m = 1 .. 64, the kernels'
    walk inside exactly-sized blocks, and regrowth that never shrinks."""
    assert "cox_score_plan_main OK pair=%d cols=%d" % (PAIR, MAXCOLS) in _run(plan_exe)


def test_layout_of_the_score_group(plan_exe):
    """Five vectors of ld doubles, three blocks of m ld, the two scans' runs per column, the centres, the two outputs, the
    partials of the pair tiles and the matrix: a partition; two flag arrays and the column indices."""
    flat = [x for case in CASES for x in case]
    for (ld, m), line in zip(CASES, _run(plan_exe, "layout", *flat).split("\n")):
        got = [int(x) for x in line.split()]
        ct = (m + PAIR - 1) // PAIR
        sizes = [ld] * 5 + [m * ld] * 3 + [2 * m * G, MAXCOLS, 2 * m * ld, G * (ct * (ct + 1) // 2) * 2 * PAIR * PAIR, m * m]
        want, at = [], 0
        for s in sizes:
            want.append(at)
            at += s
        assert got[:13] == want and got[13] == at, (ld, m)
        assert got[14:] == [0, 2 * G, 2 * G + MAXCOLS]
