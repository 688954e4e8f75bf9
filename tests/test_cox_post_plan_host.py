"""What csrc/cox_plan.hpp adds for the post-estimation exports, without a GPU: the post group's layout (cox_post_layout), the
earlier layouts value for value what they were, and the table's compaction -- the runs' records, the two scans, the slots -- as
a stand-alone program under the host sanitizers (tests/cox_post_plan_main.cpp) and against a Python restatement of the layout
at ld = 32, T, T + 32 and 5 T + 32."""
import os
import subprocess

import pytest

import _cox_plan as CP

HERE = os.path.dirname(os.path.abspath(__file__))
T = CP.TILE
LDS = (32, T, T + 32, 5 * T + 32)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coxp") / "cox_post_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cox_post_plan_main.cpp")], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


def test_layouts_walk_and_the_compaction(plan_exe):
    """Includes: cox_layout and cox_efron_layout are unchanged at ld = 32 and 4096."""
    assert "cox_post_plan_main OK tile=1024" in _run(plan_exe)


def test_layout_of_the_post_group(plan_exe):
    """dv, flag and five columns of ld doubles back to back, the two scans' runs and the count behind them; the stratum column, slotpos and
    one flag array: a partition, nothing overlaps and nothing is unused."""
    G = CP.MAX_GRID
    for ld, line in zip(LDS, _run(plan_exe, "layout", *LDS).split("\n")):
        got = [int(x) for x in line.split()]
        assert got == [0, ld, 2 * ld, 7 * ld, 7 * ld + 2 * G, 7 * ld + 2 * G + 1, 0, ld, 2 * ld, 2 * ld + G], ld
        dv, flag, out, sums, total, doubles, stratum, slotpos, heads, ints = got
        spans = sorted([(dv, dv + ld), (flag, flag + ld)] + [(out + c * ld, out + (c + 1) * ld) for c in range(5)]
                       + [(sums + i * G, sums + (i + 1) * G) for i in range(2)] + [(total, total + 1)])
        assert spans[0][0] == 0 and spans[-1][1] == doubles
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert (stratum, slotpos, heads, ints) == (0, ld, 2 * ld, 2 * ld + G)
