"""The on-chip edge cases (tests/_onchip_edge_cases.py) are decided away from rounding -- checked on the oracle alone, no GPU.

k_solve_small visits in covariance form (g <- g - h G_k), the oracle on the residual, so the two round differently.  Holding
the kernel to the oracle's pass counts, visit counts and support ORDER is only fair where the oracle's own outcome does not
hang on the last bits: every case is run as given and on three copies whose X and y carry independent relative 1e-13 noise
-- a thousand times the rounding either side commits -- and all four runs must agree on every discrete outcome at every
lambda.  No case is exempt; one that fails here gets another seed before a GPU sees it.  One that passes here and differs on
the GPU is a finding about the kernel."""
import numpy as np
import pytest

import _onchip_edge_cases as E
import _small_plan as SP


@pytest.mark.parametrize("case", E.ALL, ids=[c.id for c in E.ALL])
def test_discrete_outcomes_survive_relative_1e13_noise(case):
    want = E.oracle_of(case)
    for copy in (1, 2, 3):
        got = E.run_oracle(case, E.perturbed(case, copy), opt_tol=1e-10 if case.f32 else None)
        assert E.discrete(got) == E.discrete(want), (case.id, copy)
        for a, b in zip(got["solves"], want["solves"]):                  # and the iterate moves with the data, no further
            assert np.max(np.abs(a["beta"] - b["beta"])) <= 1e-10 * max(1.0, np.max(np.abs(b["beta"])))


@pytest.mark.parametrize("case", E.ALL, ids=[c.id for c in E.ALL])
def test_each_case_reaches_the_edge_it_is_there_for(case):
    E.check_design(case)


def test_the_case_list_is_the_issues():
    ids = set(E.BY_ID)
    for p in (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024):
        for loss in ("ls", "sqrt"):
            for order in ("ordered", "shuffled"):
                c = E.BY_ID[f"{loss}-p{p}-{order}"]
                assert (c.n, c.s, len(c.fractions)) == (max(300, min(1500, 2 * p)), min(p // 2, 120), 3) and c.warm
                assert c.n * c.p * 8 < 16 << 20                          # the Gram form is built at the first solve
    assert {f"wls-p{p}-shuffled" for p in (65, 513, 1024)} <= ids and "ls-p1024-cold-shuffled" in ids
    assert {c.p for c in E.CUT} == {513, 1024} and all(c.max_iter == 3 for c in E.CUT)
    assert {c.x0 for c in E.DROPZEROS} >= {"small150", "small70"} and {c.randomize for c in E.DROPZEROS} == {False, True}
    assert {(c.loss, c.entry) for c in E.LONG_WARM} == {("ls", "cd"), ("ls", "solve"), ("sqrt", "cd"), ("sqrt", "solve")}
    assert {c.p for c in E.F32} == {513, 1024} and len(E.OFF_CHIP) == 8
    # every unroll width, both kernels (least squares, sqrt-lasso), ordered and shuffled
    assert {(SP.unroll(c.p), c.loss == "sqrt", c.randomize) for c in E.MATRIX} == {(w, s, r) for w in (4, 8, 16) for s in (False, True)
                                                                                   for r in (False, True)}
