"""The cache-served full pass the host drives, at its block, window and scan-loop edges: gc_pass_device and the windowed walk of
gc_full_pass (csrc/grad_cache.hpp) with k_cov_scan, k_cov_block<NG>, k_cov_gupdate_chk, k_cov_restore and k_cov_pack
(csrc/gram_kernels.hpp), on the constructed cases of tests/_cov_pass_cases.py -- designs whose Gram matrix is known entry by
entry, so that a certificate breaks at a chosen position of a chosen block's window, or must NOT be flagged because its mover
comes after it.  tests/test_cov_pass_cases_host.py shows on the CPU that every case is what it declares and that none of it
hangs on the last bits.

Every case goes pass by pass through cdPass_ (gradient cache 3, screening 2, the one-launch solve off) against the oracle's
cdPass_: the iterate within BETA_TOL, maxH, the support's order, the residual at the end; between passes the counters must move as
the oracle's account of the pass says -- forced rounds, rollbacks, visits, whether the pass completed on the device.  Then the
whole list again with every device pass declared failed (the windowed walk takes each pass), groups a and c in fp32 storage, and
the cases as warm-started solves with the pass loop on the device (no helpers) and on the host."""
import functools

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _cov_pass_cases as K

pytestmark = pytest.mark.gpu

BETA_TOL = 1e-10
F32_TOL = 3e-4                  # test_gradient_cache_serves_fp32_storage: fp32 storage against the fp64 oracle
F32_RESID_TOL = 2e-3            # the same test's bar on the caught-up fp32 residual
IDS = [c.id for c in K.ALL]


def _handle(case, f32=False):
    X, y = K.data(case)
    if f32:
        X, y = np.asfortranarray(X.astype(np.float32)), y.astype(np.float32)
    f, g, x = K.make(cd, case, X, y)
    f.set_gradient_cache(3)
    f.set_screening(2)
    f.set_onchip_solve(False)
    if case.mode[0] == "block":
        f.set_sweep_mode("block", case.mode[1])
    else:
        f.set_sweep_mode("coord")
    return f, g, x


def _counters(f):
    cs, dl = f.cache_stats(), f.device_loop_stats()
    return {"passes": cs["passes"], "device": cs["device_passes"], "exact": cs["exact_visits"], "settled": cs["settled_visits"],
            "rollbacks": cs["rollbacks"], "forced": dl["forced_rounds"]["host_pass"], "launches": dl["launches"]}


def _walk_passes(case, f32=False):
    """-> per pass (maxH, beta, support, counter deltas), and the residual at the end"""
    f, g, x = _handle(case, f32)
    try:
        cd.initialize_(f, x)
        out, before = [], _counters(f)
        for lst in case.lists:
            mh = cd.cdPass_(x, f, g, lst + 1)
            after = _counters(f)
            out.append((mh, x.dense().copy(), np.asarray(x.nzval2ind).tolist(), {k: after[k] - before[k] for k in after}))
            before = after
        return out, np.array(f.r, dtype=np.float64)
    finally:
        f.close()


def _hold_iterates(case, got, r, tol=BETA_TOL, exact=True):
    """exact=False (fp32 storage): the iterate within `tol`, maxH to fp32's precision, the caught-up residual within F32_RESID_TOL"""
    want = K.oracle_of(case)
    for n, ((mh, beta, sup, d), ps) in enumerate(zip(got, want["passes"])):
        print(f"{case.id} pass {n + 1}: |beta - oracle| = {np.max(np.abs(beta - ps['beta'])):.3e} maxH {mh:.17g} / {ps['maxH']:.17g} "
              f"nnz {len(sup)} / {len(ps['support'])} counters {d}  oracle: U {int(np.count_nonzero(ps['uns_scan']))} "
              f"V {len(ps['V'])} rounds {ps['rounds']}")
    print(f"{case.id}: |r - oracle| = {np.max(np.abs(r - want['r'])):.3e}")
    for n, ((mh, beta, sup, d), ps) in enumerate(zip(got, want["passes"])):
        np.testing.assert_allclose(beta, ps["beta"], rtol=0, atol=tol, err_msg=f"{case.id} pass {n + 1}")
        assert sup == ps["support"], (case.id, n + 1)
        if exact:
            np.testing.assert_allclose(mh, ps["maxH"], rtol=1e-8, atol=1e-13, err_msg=f"{case.id} pass {n + 1}")
        else:
            np.testing.assert_allclose(mh, ps["maxH"], rtol=2.0 ** -20, atol=tol, err_msg=f"{case.id} pass {n + 1}")
    np.testing.assert_allclose(r, want["r"], rtol=0, atol=1e-9 if exact else F32_RESID_TOL, err_msg=case.id)


def _expected(case, n, ps):
    """(served, device, forced rounds, rollbacks or None where the walk's own are not declared) of pass n (0-based)"""
    lst = ps["lst"]
    if not case.served and n < 2:                   # the back-off, and the one plain pass it asks for (gc_back_off)
        return False, False, 0, 0
    if n == 0 and case.nnz0 == 0:                   # no Gram column, so no device store yet: the walk fetches and serves the pass
        return True, False, 0, 0
    zero_settled = bool(np.any((ps["g_scan"][lst] == 0.0) & ~ps["uns_scan"]))
    if zero_settled:
        return True, False, 0, None
    if ps["rounds"] > K.MAX_FORCED_ROUNDS:
        return True, False, K.MAX_FORCED_ROUNDS, None
    return True, True, ps["rounds"], 0


def _hold_counters(case, got):
    want = K.oracle_of(case)
    for n, ((_, _, _, d), ps) in enumerate(zip(got, want["passes"])):
        m = len(ps["lst"])
        served, device, forced, rollbacks = _expected(case, n, ps)
        if n == 0:                                   # what the case declares, spelled out
            assert (served, device, forced) == (case.served, case.device, case.forced_rounds)
            rollbacks = case.rollbacks
        where = (case.id, n + 1, d)
        assert d["launches"] == 0, where
        assert d["passes"] == (1 if served else 0) and d["device"] == (1 if device else 0), where
        assert d["forced"] == forced, where
        if rollbacks is not None:
            assert d["rollbacks"] == rollbacks, where
        assert d["exact"] + d["settled"] == (m if served else 0), where
        if device:
            assert d["exact"] == len(ps["visited"]) == len(ps["V"]), where


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_pass_by_pass_against_the_oracle(case):
    got, r = _walk_passes(case)
    _hold_iterates(case, got, r)
    _hold_counters(case, got)


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_every_pass_through_the_windowed_walk(case, monkeypatch):
    """CDH_GC_INJECT_ROLLBACK=1: every device pass is declared failed after it ran, undone, and walked in windows"""
    monkeypatch.setenv("CDH_GC_INJECT_ROLLBACK", "1")
    got, r = _walk_passes(case)
    _hold_iterates(case, got, r)
    for n, (_, _, _, d) in enumerate(got):
        assert d["device"] == 0 and d["launches"] == 0 and d["forced"] == 0, (case.id, n + 1, d)
        assert d["exact"] + d["settled"] == (len(case.lists[n]) if d["passes"] else 0), (case.id, n + 1, d)
    if case.walk_break:                               # a window of the walk was re-run: more than the injected rollback
        assert got[0][3]["rollbacks"] > 1, (case.id, got[0][3])


@pytest.mark.parametrize("case", K.F32, ids=[c.id for c in K.F32])
def test_fp32_storage(case):
    """groups a and c in fp32 storage (their data is exact in fp32, the margins clear the certificates' fp32 allowance a
    hundredfold: test_margins_in_every_pass), so the counts hold as in fp64"""
    got, r = _walk_passes(case, f32=True)
    _hold_iterates(case, got, r, tol=F32_TOL, exact=False)
    _hold_counters(case, got)


# ---- the same cases as warm-started solves ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solved(case, loop):
    f, g, x = _handle(case)
    try:
        if loop:
            f.set_device_loop(True, helpers=0)
        else:
            f.set_device_loop(False)
        cd.coordinateDescent_(x, f, g, cd.CDOptions(maxIter=500, optTol=1e-10, randomize=False, warmStart=True))
        st, cs, dl = f.last_stats, f.cache_stats(), f.device_loop_stats()
        broke = cs["rollbacks"] + dl["forced_rounds"]["host_pass"] + dl["forced_rounds"]["loop"]
        return x.dense().copy(), st["passes"], st["visits"], bool(st["converged"]), np.asarray(x.nzval2ind).tolist(), broke
    finally:
        f.close()


@pytest.mark.parametrize("loop", [True, False], ids=["device-loop", "host-loop"])
@pytest.mark.parametrize("case", K.SOLVES, ids=[c.id for c in K.SOLVES])
def test_warm_started_solves(case, loop):
    got, want = _solved(case, loop), K.solve_oracle(case)
    print(f"{case.id}: |beta - oracle| = {np.max(np.abs(got[0] - want[0])):.3e} passes {got[1]} / {want[1]} visits {got[2]} / {want[2]} "
          f"converged {got[3]} / {want[3]} broken certificates met {got[5]}")
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=BETA_TOL, err_msg=case.id)
    assert got[1:5] == want[1:5], case.id


def test_the_solves_met_broken_certificates():
    assert sum(_solved(case, loop)[5] for case in K.SOLVES for loop in (True, False)) > 0
