"""k_solve_small (csrc/small_solve.hpp) at its chunk, unroll and column-cache edges.  The cases, what each is there for and the
one helper that runs them are tests/_onchip_edge_cases.py's; tests/test_onchip_edge_cases_host.py has shown, without a GPU,
that every case's discrete outcome survives relative 1e-13 noise on X and y -- so a difference here is the kernel's.

The bar is tests/test_gpu_onchip_solve.py's: beta within 1e-10 max(1, |beta|_inf) of the oracle at every lambda, the same
passes, visits, converged and support ORDER (the order is the visit order of the next active pass), f.r within 1e-9 of the
oracle's residual at the end, and onchip_stats() counting every solve on ONE Gram matrix -- the kernel under test is what ran.

What goes wrong where (each seen to fail by breaking the kernel on purpose, LAB_NOTES "On-chip edges"):
  * the clamp min(lane + 64 t, p - 1) / the store predicate lane + 64 t < p: p = 257, 513, 1000 -- a read or write past the
    vector's end lands in the neighbouring LDS array (beta, or the first cached column);
  * keep == false (the column cache full): every p >= 256 case, whose support outgrows ncache(p) -- moves then mix both branches;
  * the L <= 64 switch of wave_build_list: the shuffled cases whose support crosses 64 (p >= 128);
  * wave_dropzeros' chunk loops: the ls-p300-small* cases (150, 70 and 200 slots, holes and fillers in different chunks) --
    the support ORDER afterwards is the assertion that bites."""
import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _onchip_edge_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _onchip(monkeypatch):
    monkeypatch.setenv("CDH_SMALL_PATH", "1")


_ON_CHIP = {}                    # case id -> the one-launch run (filled by the first test; the off-chip test compares with it)


def _on_chip(case):
    if case.id not in _ON_CHIP:
        _ON_CHIP[case.id] = E.run_device(cd, case)
    return _ON_CHIP[case.id]


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", E.EXACT, ids=_ids(E.EXACT))
def test_one_launch_solve_is_the_oracles(case):
    E.check_design(case)
    got = _on_chip(case)
    E.hold_to(got, E.oracle_of(case), case)
    assert got["stats"] == {"solves": E.n_solves(case), "gram_matrices": 1}


@pytest.mark.parametrize("case", E.F32, ids=_ids(E.F32))
def test_fp32_storage_at_the_widest_kernel(case):
    """fp32 X and y, the device's optTol = 1e-6, against the fp64 oracle (optTol 1e-10) on the fp32-rounded inputs: beta within
    3e-4.  Nothing discrete is asserted for fp32, as elsewhere in the suite."""
    E.check_design(case)
    got = E.run_device(cd, case)
    E.hold_to(got, E.oracle_of(case), case, exact=False)
    assert got["stats"] == {"solves": E.n_solves(case), "gram_matrices": 1} and got["r"].dtype == np.float32


@pytest.mark.parametrize("case", E.OFF_CHIP, ids=_ids(E.OFF_CHIP))
def test_same_answer_off_the_chip(case):
    """The same path on the streamed per-coordinate sweep: beta within 1e-10 of the one-launch solve's, the same orders and
    counts (and the oracle's), and no one-launch solve counted."""
    got, on = E.run_device(cd, case, onchip=False), _on_chip(case)
    assert got["stats"] == {"solves": 0, "gram_matrices": 0} and on["stats"]["solves"] == E.n_solves(case)
    E.hold_to(got, E.oracle_of(case), case)
    assert E.discrete(got) == E.discrete(on)
    for a, b in zip(got["solves"], on["solves"]):
        np.testing.assert_allclose(a["beta"], b["beta"], rtol=0, atol=E.BETA_TOL * max(1.0, float(np.max(np.abs(b["beta"])))))
