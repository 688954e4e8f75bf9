"""What csrc/cox_plan.hpp adds for Efron ties, without a GPU: the Efron pair's layout (cox_efron_layout), the strata bounds a
plain handle gets when it turns to Efron (cox_one_stratum), and the runs' records of the tie-group scans -- as a stand-alone
program under the host sanitizers (tests/cox_efron_plan_main.cpp) and against Python restatements at ld = 32, T, T + 32 and
5 T + 32."""
import os
import subprocess

import numpy as np
import pytest

import _cox_plan as CP
import _cox_strata_numpy as CS

HERE = os.path.dirname(os.path.abspath(__file__))
T = CP.TILE
LDS = (32, T, T + 32, 5 * T + 32)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coxe") / "cox_efron_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cox_efron_plan_main.cpp")], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


def test_layout_walk_and_the_tie_group_records(plan_exe):
    assert "cox_efron_plan_main OK tile=1024" in _run(plan_exe)


def test_layout_of_the_efron_pair(plan_exe):
    """Seven vectors of ld doubles back to back, the five scans' runs behind them, two flag arrays: no two overlap, and the
    pairs that one launch scans together are ld (their runs MAX_GRID) apart."""
    G = CP.MAX_GRID
    for ld, line in zip(LDS, _run(plan_exe, "layout", *LDS).split("\n")):
        got = [int(x) for x in line.split()]
        assert got == [0, ld, 2 * ld, 3 * ld, 4 * ld, 5 * ld, 6 * ld, 7 * ld, 7 * ld + 5 * G, 0, G, 2 * G], ld
        cnt, Dv, Sdv, hc, hc2, lg, mm, sums, doubles = got[:9]
        spans = sorted([(o, o + ld) for o in (cnt, Dv, Sdv, hc, hc2, lg, mm)] + [(sums + i * G, sums + (i + 1) * G) for i in range(5)])
        assert spans[0][0] == 0 and spans[-1][1] == doubles
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))          # a partition: nothing overlaps, nothing is unused
        assert Dv - cnt == ld and hc2 - hc == ld


@pytest.mark.parametrize("ld", LDS)
def test_one_stratum_is_the_order_without_ids(plan_exe, ld):
    """cox_one_stratum(n, ld) for the n that pad to ld: the rows one stratum, the pads another -- the twin's bounds without
    strata, and the pads as cox_order_strata leaves them."""
    for n in sorted({max(ld - 31, 1), ld - 1, ld}):
        sfirst, slast = (np.array(line.split(), dtype=np.int64) for line in _run(plan_exe, "stratum", n).split("\n")[:2])
        assert sfirst.shape == slast.shape == (ld,)
        _, _, _, sf, sl = CS.groups(np.arange(n, dtype=np.float64) % 3, None)
        np.testing.assert_array_equal(sfirst[:n], sf)
        np.testing.assert_array_equal(slast[:n], sl)
        np.testing.assert_array_equal(sfirst[n:], n)
        np.testing.assert_array_equal(slast[n:], ld - 1)
