"""The constructed cases of tests/_cov_pass_cases.py are what they declare -- checked on the oracle alone, no GPU.

tests/test_gpu_cov_pass_edges.py asserts counts: how often gc_pass_device ran a pass again, how many positions it visited,
whether it finished on the device.  Those are only a fair demand where the oracle itself says so and where nothing hangs on the
last bits.  Every case is therefore walked visit by visit on the oracle, X_k'W r taken at each coordinate's turn:
  - who is unsettled at the scan (cov_settled's rule: beta != 0 or |g| > thr (1 - 1e-9)) and who at its turn,
  - the rounds gc_pass_device needs, played with the oracle's own visits (the chain length),
  - every |g_k| / thr_k of a coordinate at zero at least 5 % away from 1, at the scan and at its turn, in every pass, and further away
    than the allowance fp32 storage adds to a certificate,
  - no g0_k exactly zero except where declared,
and all of it once more on three copies whose X and y carry relative 1e-13 noise: the discrete outcomes must not change."""
import numpy as np
import pytest

import _cov_pass_cases as K
import oracle as O

IDS = [c.id for c in K.ALL]


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_pass_one_is_what_the_case_declares(case):
    tr = K.oracle_of(case)
    p1 = tr["passes"][0]
    lst = p1["lst"]
    assert len(np.unique(lst)) == len(lst) >= 16 and case.nnz0 * 4 <= case.p        # the pass is offered to the cache at all
    assert int(np.count_nonzero(p1["uns_scan"])) == case.U, case.id
    broke = tuple(np.flatnonzero(p1["uns_turn"] & ~p1["uns_scan"]))
    assert broke == tuple(sorted(case.breaks)), (case.id, broke)
    assert sorted(p1["V"]) == sorted(set(np.flatnonzero(p1["uns_scan"])) | set(case.breaks))
    assert list(p1["visited"]) == list(p1["V"]), case.id                             # no round marks a coordinate that stays put
    chain = p1["rounds"]
    assert min(chain, K.MAX_FORCED_ROUNDS) == case.forced_rounds, (case.id, chain)
    assert (chain > K.MAX_FORCED_ROUNDS) == (case.rollbacks > 0), (case.id, chain)
    g0 = p1["g_scan"]
    assert tuple(np.flatnonzero(g0 == 0.0)) == tuple(sorted(case.zero_g)), case.id
    # entering coordinates: unsettled at the scan with beta = 0 (no Gram column yet: nothing has fetched one)
    entering = int(np.count_nonzero(p1["uns_scan"] & (p1["beta_scan"][lst] == 0.0)))
    assert case.served == (entering <= K.GC_BUSY), case.id
    # (a handle without any Gram column yet has no device store: gc_pass_device leaves its first pass to the walk)
    assert case.device == (case.served and not case.zero_g and chain <= K.MAX_FORCED_ROUNDS and case.nnz0 > 0), case.id


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_margins_in_every_pass(case):
    X, y = K.data(case)
    w = np.ones(case.p) if case.w is None else case.w
    a = np.einsum("ij,ij->j", X, X * w[:, None])
    allowance = K.gc_cert_abs(case, y) * np.sqrt(a)
    for n, ps in enumerate(K.oracle_of(case)["passes"]):
        lst = ps["lst"]
        at_zero = ps["beta_scan"][lst] == 0.0
        for what, g, thr in (("scan", ps["g_scan"][lst], ps["thr_scan"][lst]), ("turn", ps["g_turn"], ps["thr_turn"])):
            ratio = np.abs(g[at_zero]) / thr[at_zero]
            assert np.all(np.abs(ratio - 1.0) >= 0.05), (case.id, n, what, ratio[np.abs(ratio - 1.0) < 0.05])
            if case.f32:
                room = np.abs(np.abs(g[at_zero]) - thr[at_zero])
                assert np.all(room > 100.0 * allowance[lst][at_zero]), (case.id, n, what)
    if case.f32:                                      # fp32 storage holds the same problem: the fp64 oracle is its reference as it stands
        assert np.array_equal(X.astype(np.float32), X) and np.array_equal(y.astype(np.float32), y), case.id


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_discrete_outcomes_survive_relative_1e13_noise(case):
    want = K.oracle_of(case)
    for copy in (1, 2, 3):
        got = K.trace(case, *K.perturbed(case, copy))
        assert K.discrete(got) == K.discrete(want), (case.id, copy)
        for a, b in zip(got["passes"], want["passes"]):
            assert np.max(np.abs(a["beta"] - b["beta"])) <= 1e-10 * max(1.0, np.max(np.abs(b["beta"])))


@pytest.mark.parametrize("case", K.SOLVES, ids=[c.id for c in K.SOLVES])
def test_solves_survive_relative_1e13_noise(case):
    want = K.solve_oracle(case)
    assert want[3], case.id
    for copy in (1, 2, 3):
        got = K.solve_oracle(case, *K.perturbed(case, copy))
        assert got[1:] == want[1:], (case.id, copy)
        assert np.max(np.abs(got[0] - want[0])) <= 1e-10 * max(1.0, np.max(np.abs(want[0])))


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_the_trace_is_the_oracles_pass(case):
    """visit by visit and dropzeros! at the end is what cdPass_ does: same iterate, same support order, same maxH"""
    X, y = K.data(case)
    f, g, x = K.make(O, case, X, y)
    O.initialize_(f, x)
    for lst, ps in zip(case.lists, K.oracle_of(case)["passes"]):
        mh = O.cdPass_(x, f, g, lst + 1)
        assert np.array_equal(x.dense(), ps["beta"]) and np.asarray(x.nzval2ind).tolist() == ps["support"] and mh == ps["maxH"]
    if case.still:
        assert np.all(K.oracle_of(case)["passes"][1]["h"] == 0.0) and np.any(K.oracle_of(case)["passes"][0]["h"] != 0.0)
    if case.loss != "sqrt":                            # the construction is exact: X'W r0 is the gradient that was asked for
        w = np.ones(case.p) if case.w is None else case.w
        a = np.einsum("ij,ij->j", X, X * w[:, None])
        assert np.array_equal(K.oracle_of(case)["passes"][0]["g_scan"], X.T @ (w * case.r0))
        assert np.all(a > 0)


def test_the_case_list_is_the_issues():
    ids = set(K.BY_ID)
    for mode in ("coord0", "block16", "block32", "block64"):
        B = 16 if mode == "coord0" else int(mode[5:])
        for U in (1, B - 1, B, B + 1, 2 * B, 2 * B + 1):
            c = K.BY_ID[f"a-{mode}-U{U}"]
            assert c.U == U and K.width(c.mode) == B and c.still and len(c.lists) == 2
    assert {K.width(c.mode) for c in K.Bg} == {16, 32, 64} and all(c.U == 2 * K.width(c.mode) + 1 for c in K.Bg)
    for name in ("inside", "between", "last-1", "prev+1"):
        assert {f"b-{name}-break", f"b-{name}-mirror"} <= ids
        assert K.BY_ID[f"b-{name}-mirror"].forced_rounds == 0 and K.BY_ID[f"b-{name}-break"].forced_rounds == 1
    assert K.BY_ID["b-tail-end-break"].breaks == (271,) and K.BY_ID["b-before-first-visit"].breaks == ()
    assert {c.p for c in K.Cg if c.id.startswith("c-scan")} == {1023, 1024, 1025, 2049}
    big = K.oracle_of(K.BY_ID["c-scan-p2049"])["passes"][0]
    assert {1022, 1023, 1024, 1025, 2047, 2048} <= set(np.flatnonzero(big["uns_scan"]))
    assert {c.p for c in K.D} == {255, 256, 257}
    assert {c.loss for c in K.E} == {"ls", "wls", "sqrt"}
    assert [c.forced_rounds for c in K.F] == [1, 2, 3, 4, 4] and [c.rollbacks for c in K.F] == [0, 0, 0, 0, 1]
    assert [c.U - c.nnz0 for c in K.G] == [64, 65, 64, 2] and [(c.served, c.device) for c in K.G] == [(True, True), (False, False), (True, False), (True, False)]
    assert max(c.p for c in K.ALL) == 2049 and all(c.walk_break for c in K.W)
