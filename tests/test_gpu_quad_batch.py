"""CDQuadraticLoss batches (csrc/quad_solve.hpp, the cdh_quad exports, api.CDQuadraticLoss) wherever an index depends on the
problem's number or on a caller's list: warm batches from different non-zero iterates, cold batches with a lambda grid per
problem, shared / per-problem / mixed omega, the explicit calls on problem j of a batch, the chunk cut of the explicit pass at
its list edges, non-finite input, and seeded sequences of operations on one handle.

The reference for everything is the CPU oracle run once per problem, at the bars of test_gpu_quad.py:
beta within 1e-10, the same passes / full passes / visits / convergence flag and slot order, h and max|h| within 1e-12, the
handle's gradient within 1e-11 max(1, max|b|) of A x + b, a cold start's lambda_max at rtol 1e-15; two device runs of the same
problem (in a batch, and alone) agree bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import oracle as O
from _quad_cases import BETA_TOL, H_TOL, OPT, _A, _b, _grad_bar, _oracle_gradient, _same

pytestmark = pytest.mark.gpu

PMAX = cd.CDH_QUAD_MAX_P


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _entries(rng, p, n):
    """n (coordinate, value) assignments in a random order, the values signed: the slots they fill are not ascending."""
    ks = rng.permutation(p)[:n] + 1
    return list(zip(ks.tolist(), rng.standard_normal(n).tolist()))


def _pair(p, entries):
    """The same iterate on both sides, built by the same assignments in the same order."""
    x, xo = cd.SparseIterate(p), O.SparseIterate(p)
    for k, v in entries:
        x[k] = v
        xo[k] = v
    assert x.nzval2ind.tolist() == xo.nzval2ind.tolist()
    return x, xo


def _batch_starts(rng, p, m, cap=None):
    """Problem 0 empty, problem 1 dense (or `cap` entries), the rest of random density."""
    full = p if cap is None else cap
    return [_entries(rng, p, 0 if j == 0 else full if j == 1 else int(rng.integers(1, full))) for j in range(m)]


def _grad_check(f, j, x, b, tag=""):
    np.testing.assert_allclose(f._gradient_vector(j), _A(f.p) @ x.dense() + b, rtol=0, atol=_grad_bar(b), err_msg=str(tag))


def _bits(x):
    return x.dense().tobytes(), x.nzval2ind.tolist()


# ---- 1. warm batches from non-zero, different iterates -----------------------------------------------------------------------
def _warm_batch(p, m, rand, B, lams, starts):
    A = _A(p)
    opts = dict(OPT, warmStart=True, randomize=rand, seed=3)
    f = cd.CDQuadraticLoss(A, B, max_batch=m)
    pairs = [_pair(p, e) for e in starts]
    if p < 1024:
        assert pairs[0][0].nnz == 0 and pairs[1][0].nnz == p
        assert any(np.any(np.diff(x.nzval2ind) < 0) for x, _ in pairs[1:])
    xs = [x for x, _ in pairs]
    cd.coordinateDescent_(xs, f, [cd.ProxL1(l) for l in lams], cd.CDOptions(**opts))
    alone = cd.CDQuadraticLoss(A, B[:, :1], max_batch=1)
    for j in range(m):
        fo, xo = O.CDQuadraticLoss(A, B[:, j].copy()), pairs[j][1]
        st = O.coordinateDescent_(xo, fo, O.ProxL1(lams[j]), O.CDOptions(**opts))
        assert st["converged"], j
        _same(f.last_stats[j], xs[j], st, xo, tag=j)
        _grad_check(f, j, xs[j], B[:, j], tag=j)
        # the same problem alone, from the same start: the same kernel, deterministic -> the same bits
        alone.set_b(B[:, [j]])
        x1 = [_pair(p, starts[j])[0]]
        cd.coordinateDescent_(x1, alone, cd.ProxL1(lams[j]), cd.CDOptions(**opts))
        assert _bits(x1[0]) == _bits(xs[j]), j
        assert alone.last_stats[0] == f.last_stats[j], j
        assert alone._gradient_vector(0).tobytes() == f._gradient_vector(j).tobytes(), j
    f.close()
    alone.close()


@pytest.mark.parametrize("rand", [False, True], ids=["ordered", "shuffled"])
@pytest.mark.parametrize("m", [2, 5])
@pytest.mark.parametrize("p", [40, 65, 300])
def test_warm_batch_from_different_starts(p, m, rand):
    rng = np.random.default_rng(1000 * p + 10 * m + rand)
    B = np.stack([_b(p, 400 + 7 * m + j, s=1 + j % 9) for j in range(m)], axis=1)
    lams = np.array([(0.1 + 0.12 * j) * np.abs(B[:, j]).max() for j in range(m)])     # a different lambda per problem
    _warm_batch(p, m, rand, B, lams, _batch_starts(rng, p, m))


def test_warm_batch_at_the_largest_p():
    """Three workgroups of 160 KiB of LDS each in one launch; lambda as test_single_problem_parity takes it for large p."""
    p, m = PMAX, 3
    rng = np.random.default_rng(99)
    B = np.stack([_b(p, 0), _b(p, 1), _b(p, 2)], axis=1)
    lams = np.array([float(np.sort(np.abs(B[:, j]))[-31]) for j in range(m)])
    _warm_batch(p, m, True, B, lams, _batch_starts(rng, p, m, cap=10))


# ---- 2. cold batches: a lambda grid per problem ------------------------------------------------------------------------------
P_C = 40
FRACTIONS = (0.5, 0.3, 0.2, 0.1, 0.05)


def _cold_case(m, omega):
    rng = np.random.default_rng(20 + m)
    # column j scaled by 10^j: lambda_max and the grids are orders of magnitude apart.  The whole batch is then brought down so
    # that the LARGEST problem is O(1): optTol = 1e-12 is absolute, and at |beta| ~ 1e4 it lies below one ulp of beta, where
    # the oracle itself cannot report convergence
    B = np.stack([_b(P_C, 600 + j, s=2 + j) * 10.0 ** (j - (m - 1)) for j in range(m)], axis=1)
    if omega == "none":
        oms = [None] * m
    elif omega in ("shared", "same"):
        oms = [rng.random(P_C) + 0.5] * m
    else:
        oms = [rng.random(P_C) + 0.5 for _ in range(m)]
    lmax = np.array([float((np.abs(B[:, j]) / (1.0 if oms[j] is None else oms[j])).max()) for j in range(m)])
    return B, oms, lmax, lmax * np.array(FRACTIONS[:m])


def _cold_penalty(omega, lams, oms):
    if omega == "shared":                                    # ONE ProxL1 for all: lambda0 is then shared too
        return cd.ProxL1(lams[-1], oms[0])
    return [cd.ProxL1(l, om) for l, om in zip(lams, oms)]


@pytest.mark.parametrize("omega", ["none", "shared", "same", "own"])
@pytest.mark.parametrize("steps", [1, 7, 63])
@pytest.mark.parametrize("m", [2, 5])
def test_cold_batch(m, steps, omega):
    """`shared`: a single ProxL1(l, om) for every problem (one omega on the device, ldo = 0); `same`: that vector passed once per
    problem, with a lambda0 per problem; `own`: a different omega per problem."""
    A = _A(P_C)
    B, oms, lmax, lams = _cold_case(m, omega)
    if omega == "shared":                                    # one lambda0 for all: the last problem's, at which every one converges
        lams = np.full(m, lams[-1])                          # (below lambda_max for the last two, above it for the smaller ones)
    opts = dict(OPT, warmStart=False, randomize=(steps != 7), seed=3, numSteps=steps)
    f = cd.CDQuadraticLoss(A, B)
    xs = [cd.SparseIterate(P_C) for _ in range(m)]
    cd.coordinateDescent_(xs, f, _cold_penalty(omega, lams, oms), cd.CDOptions(**opts))
    assert (f._omega is None) == (omega == "none") and (omega != "shared" or f._omega.ndim == 1)
    nnz = 0
    for j in range(m):
        fo, xo = O.CDQuadraticLoss(A, B[:, j].copy()), O.SparseIterate(P_C)
        st = O.coordinateDescent_(xo, fo, O.ProxL1(lams[j], oms[j]), O.CDOptions(**opts))
        assert st["converged"], j
        _same(f.last_stats[j], xs[j], st, xo, tag=j)
        np.testing.assert_allclose(f.last_stats[j]["lambda_max"], lmax[j], rtol=1e-15)
        _grad_check(f, j, xs[j], B[:, j], tag=j)
        nnz += xo.nnz
    assert nnz > 0
    f.close()


def test_cold_start_ignores_what_the_handle_held():
    m = 5
    A = _A(P_C)
    B, oms, _, lams = _cold_case(m, "own")
    rng = np.random.default_rng(4)
    cold = dict(OPT, warmStart=False, randomize=True, seed=3, numSteps=7)
    pens = _cold_penalty("own", lams, oms)
    fresh = cd.CDQuadraticLoss(A, B)
    xf = [cd.SparseIterate(P_C) for _ in range(m)]
    cd.coordinateDescent_(xf, fresh, pens, cd.CDOptions(**cold))
    used = cd.CDQuadraticLoss(A, B)
    xu = [_pair(P_C, e)[0] for e in _batch_starts(rng, P_C, m)]
    cd.coordinateDescent_(xu, used, [cd.ProxL1(0.02 * l) for l in lams], cd.CDOptions(**dict(OPT, warmStart=True, randomize=False)))
    assert all(x.nnz > 0 for x in xu)                        # the warm solve left non-zero results in the handle
    again = [_pair(P_C, e)[0] for e in _batch_starts(rng, P_C, m)[::-1]]    # non-empty iterates that the handle has not seen
    cd.coordinateDescent_(again, used, pens, cd.CDOptions(**cold))
    for j in range(m):
        assert _bits(again[j]) == _bits(xf[j]), j
        assert used.last_stats[j] == fresh.last_stats[j], j
        assert used._gradient_vector(j).tobytes() == fresh._gradient_vector(j).tobytes(), j
    fresh.close()
    used.close()


# ---- 3. shared and mixed omega, warm -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("omega", ["shared", "mixed"])
def test_warm_batch_shared_and_mixed_omega(omega):
    """`mixed`: problems 0 and 3 carry no omega (the binding fills in ones), the others their own."""
    p, m = 65, 5
    A = _A(p)
    rng = np.random.default_rng(33)
    B = np.stack([_b(p, 700 + j, s=2 + j) for j in range(m)], axis=1)
    if omega == "shared":
        oms = [rng.random(p) + 0.5] * m
        lams = np.full(m, 0.15 * float((np.abs(B) / oms[0][:, None]).max(axis=0).min()))
        pen = cd.ProxL1(lams[0], oms[0])
    else:
        oms = [None if j in (0, 3) else rng.random(p) * 2 + 0.25 for j in range(m)]
        lams = np.array([(0.1 + 0.05 * j) * float((np.abs(B[:, j]) / (1.0 if oms[j] is None else oms[j])).max()) for j in range(m)])
        pen = [cd.ProxL1(l, om) for l, om in zip(lams, oms)]
    opts = dict(OPT, warmStart=True, randomize=True, seed=5)
    f = cd.CDQuadraticLoss(A, B)
    pairs = [_pair(p, e) for e in _batch_starts(rng, p, m)]
    xs = [x for x, _ in pairs]
    cd.coordinateDescent_(xs, f, pen, cd.CDOptions(**opts))
    assert f._omega.ndim == (1 if omega == "shared" else 2)
    for j in range(m):
        fo, xo = O.CDQuadraticLoss(A, B[:, j].copy()), pairs[j][1]
        st = O.coordinateDescent_(xo, fo, O.ProxL1(lams[j], oms[j]), O.CDOptions(**opts))
        assert st["converged"] and xo.nnz > 0, j
        _same(f.last_stats[j], xs[j], st, xo, tag=j)
        _grad_check(f, j, xs[j], B[:, j], tag=j)
    f.close()


# ---- 4. the explicit calls on problem j of a batch ----------------------------------------------------------------------------
def _raw_state(f, j):
    """Problem j as the handle holds it: the support in slot order, its values, the gradient -- as bytes."""
    L = cd._lib.lib()
    nnz, idx, val = C.c_int64(), np.zeros(f.p, dtype=np.int64), np.zeros(f.p)
    assert L.cdh_quad_get_iterate(f._h, j, C.byref(nnz), _vp(idx), _vp(val)) == cd._lib.CDH_OK
    return idx[: nnz.value].tobytes(), val[: nnz.value].tobytes(), f._gradient_vector(j).tobytes()


@pytest.mark.parametrize("j", [0, 2, 3])
def test_explicit_calls_on_problem_j(j):
    """test_plugin_interface_call_by_call's sequence with problem=j, every other problem's iterate and gradient unchanged."""
    p, m = 65, 4
    A = _A(p)
    rng = np.random.default_rng(40 + j)
    B = np.stack([_b(p, 800 + i, s=3 + i) for i in range(m)], axis=1)
    oms = [rng.random(p) + 0.5 for _ in range(m)]
    lams = [(0.15 + 0.05 * i) * float(np.abs(B[:, i]).max()) for i in range(m)]
    f = cd.CDQuadraticLoss(A, B)
    fos = [O.CDQuadraticLoss(A, B[:, i].copy()) for i in range(m)]
    pairs = [_pair(p, _entries(rng, p, n)) for n in (20, p, 33, 48)]
    xs, xos = [x for x, _ in pairs], [xo for _, xo in pairs]
    g, go = cd.ProxL1(lams[j], oms[j]), O.ProxL1(lams[j], oms[j])
    x, xo, fo = xs[j], xos[j], fos[j]
    for i in range(m):
        cd.initialize_(f, xs[i], problem=i)
        O.initialize_(fos[i], xos[i])
    for i in range(m):
        np.testing.assert_allclose(f._gradient_vector(i), _oracle_gradient(fos[i]), rtol=0, atol=_grad_bar(B[:, i]))

    def others():
        return [_raw_state(f, i) for i in range(m) if i != j]

    def grads():
        ref = np.array([O.gradient(fo, xo, k) for k in range(1, p + 1)])
        got = np.array([cd.gradient(f, x, k, problem=j) for k in range(1, p + 1)])
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())

    before = others()
    assert len(set(before)) == m - 1
    grads()
    order = rng.permutation(np.r_[np.arange(1, p + 1), np.arange(1, p + 1)])[:40]
    moved = 0
    for k in order.tolist():
        h, ho = cd.descendCoordinate_(f, g, x, k, problem=j), O.descendCoordinate_(fo, go, xo, k)
        assert abs(h - ho) <= H_TOL, (k, h, ho)
        assert x.nzval2ind.tolist() == xo.nzval2ind.tolist()
        assert others() == before, k
        moved += ho != 0.0
    assert moved >= 10
    np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL)
    grads()
    sup = xo.nzval2ind.tolist()
    mh, mho = cd.cdPass_(x, f, g, sup, problem=j), O.cdPass_(xo, fo, go, sup)
    assert abs(mh - mho) <= H_TOL and mho > 0.0
    assert x.nzval2ind.tolist() == xo.nzval2ind.tolist() and others() == before
    twice = [3, 7, 3, 3, 9, 7] + list(range(1, p + 1)) + [p, p]
    mh, mho = cd.cdPass_(x, f, g, twice, problem=j), O.cdPass_(xo, fo, go, twice)
    assert abs(mh - mho) <= H_TOL and x.nzval2ind.tolist() == xo.nzval2ind.tolist()
    assert others() == before
    np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL)
    grads()
    _grad_check(f, j, x, B[:, j])
    np.testing.assert_allclose(cd.findLambdaMax(x, f, g, problem=j), O.findLambdaMax(xo, fo, go), rtol=1e-12)
    np.testing.assert_allclose(cd.objective(f, g, problem=j), O.objective(fo, go, xo), rtol=1e-12)
    assert others() == before
    # and what the handle holds for problem j is what the binding handed back
    idx, val, _ = _raw_state(f, j)
    assert idx == x.nzval2ind.astype(np.int64).tobytes() and val == x.nzval.tobytes()
    f.close()


# ---- 5. list edges of the explicit pass --------------------------------------------------------------------------------------
P_L = 130


def _lists():
    perm = (np.random.default_rng(5).permutation(P_L) + 1).tolist()
    return {
        "len0": [], "len1": perm[:1], "len64": perm[:64], "len65": perm[:65], "len128": perm[:128], "len129": perm[:129],
        "repeat_opens_next_chunk": list(range(1, 65)) + [1],
        "repeat_at_lane63": list(range(1, 64)) + [1],
        "repeat_at_lane1": [5, 5] + list(range(6, 70)),
        "one_coordinate": [17] * 130,
        "pairs": [k for k in perm[:70] for _ in (0, 1)],
        "perm_then_reverse": perm + perm[::-1],
    }


LISTS = _lists()


@functools.lru_cache(maxsize=None)
def _list_problem():
    rng = np.random.default_rng(55)
    b = _b(P_L, 900, s=12)
    x0 = np.where(rng.random(P_L) < 0.6, rng.standard_normal(P_L), 0.0)        # 60 % dense, signed
    entries = [(int(k) + 1, float(x0[k])) for k in rng.permutation(P_L) if x0[k] != 0.0]
    return b, entries


@pytest.fixture
def list_handle():
    f = cd.CDQuadraticLoss(_A(P_L), _list_problem()[0])
    yield f
    f.close()


def _list_state(f, regime):
    """Both sides at the regime's start, and its lambda.  `half` and `all` start from the 60 % dense iterate; `none` from what a
    pass at a huge lambda leaves of it: an empty iterate whose gradient is the carried one, under a lambda above findLambdaMax,
    so that a visit moves nothing, stores a zero where x_k - g_k / A_kk is not zero, and dropzeros! takes it out again."""
    b, entries = _list_problem()
    fo = O.CDQuadraticLoss(_A(P_L), b)
    x, xo = _pair(P_L, entries)
    cd.initialize_(f, x)
    O.initialize_(fo, xo)
    lmax = O.findLambdaMax(xo, fo, O.ProxL1(1.0))
    if regime == "all":
        return fo, b, x, xo, 0.0
    if regime == "half":
        return fo, b, x, xo, 0.9 * lmax
    huge, every = 1e6 * lmax, list(range(1, P_L + 1))
    mh, mho = cd.cdPass_(x, f, cd.ProxL1(huge), every), O.cdPass_(xo, fo, O.ProxL1(huge), every)
    assert abs(mh - mho) <= H_TOL and x.nnz == xo.nnz == 0
    return fo, b, x, xo, 1.5 * O.findLambdaMax(xo, fo, O.ProxL1(1.0))


def _count_moves(fo, go, xo, lst):
    """The oracle's own count of the visits of `lst` that move, and of the slots they leave, on a copy of its state."""
    fc, xc = O.CDQuadraticLoss(fo.X, fo.y), xo.copy()
    fc.r[:] = fo.r
    moves = sum(O.descendCoordinate_(fc, go, xc, k) != 0.0 for k in lst)
    return moves, xc.nnz


def _check_regime_counts(regime, lst, moves, slots):
    distinct = len(set(lst))
    if regime == "none":
        assert moves == 0 and slots == distinct              # nothing moves; every coordinate visited is stored as a zero
    elif regime == "all":
        assert moves >= distinct and (moves == len(lst) or distinct < len(lst))     # lambda = 0: a first visit always moves
    elif distinct == len(lst) >= 64:
        # the stored 60 % always move (x_k - g_k / A_kk is generically not x_k), the empty 40 % almost never at 0.9 lambda_max
        assert 0.45 * len(lst) <= moves <= 0.75 * len(lst), (moves, len(lst))


@pytest.mark.parametrize("regime", ["half", "none", "all"])
@pytest.mark.parametrize("name", list(LISTS))
def test_explicit_pass_list_edges(list_handle, name, regime):
    lst, f = LISTS[name], list_handle
    fo, b, x, xo, lam = _list_state(f, regime)
    g, go = cd.ProxL1(lam), O.ProxL1(lam)
    moves, slots = _count_moves(fo, go, xo, lst)
    _check_regime_counts(regime, lst, moves, slots)
    mh, mho = cd.cdPass_(x, f, g, lst), O.cdPass_(xo, fo, go, lst)
    assert abs(mh - mho) <= H_TOL, (mh, mho)
    assert (mho > 0.0) == (moves > 0)
    np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL)
    assert x.nzval2ind.tolist() == xo.nzval2ind.tolist()
    np.testing.assert_allclose(f._gradient_vector(0), _oracle_gradient(fo), rtol=0, atol=_grad_bar(b))
    if regime != "none":                                     # (`none` carries its gradient from the pass that emptied x)
        _grad_check(f, 0, x, b)


@pytest.mark.parametrize("regime", ["half", "none"])
@pytest.mark.parametrize("name", list(LISTS))
def test_explicit_lists_call_by_call(list_handle, name, regime):
    """The same lists through descendCoordinate_: no dropzeros! on this path, so stored zeros keep the oracle's slots."""
    lst, f = LISTS[name], list_handle
    fo, b, x, xo, lam = _list_state(f, regime)
    g, go = cd.ProxL1(lam), O.ProxL1(lam)
    for t, k in enumerate(lst):
        h, ho = cd.descendCoordinate_(f, g, x, k), O.descendCoordinate_(fo, go, xo, k)
        assert abs(h - ho) <= H_TOL, (t, k, h, ho)
        assert x.nzval2ind.tolist() == xo.nzval2ind.tolist(), (t, k)
    if regime == "none" and lst:
        assert x.nnz == len(set(lst)) and not x.dense().any()               # stored zeros, all of them still in their slots
    np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL)
    np.testing.assert_allclose(f._gradient_vector(0), _oracle_gradient(fo), rtol=0, atol=_grad_bar(b))


@functools.lru_cache(maxsize=None)
def _repeat_case():
    """From the oracle alone: on the empty iterate (g = b), j = argmax |b| and a k and lambda with |b_k| <= lambda < |b_j| such
    that k settles as a stored zero while j has not moved, and moves to a non-zero once j has.  Returns 1-based j, k, lambda and
    the coordinates that settle whatever j does (|b| well below lambda)."""
    b = _list_problem()[0]
    order = np.argsort(-np.abs(b))
    j = int(order[0])
    for k in order[1:12].tolist():
        for lam in np.linspace(abs(b[k]) * 1.0001, abs(b[j]) * 0.999, 400).tolist():
            fo, xo = O.CDQuadraticLoss(_A(P_L), b), O.SparseIterate(P_L)
            O.initialize_(fo, xo)
            hs = [O.descendCoordinate_(fo, O.ProxL1(lam), xo, c + 1) for c in (k, k, j, k)]
            if hs[0] == 0.0 and hs[1] == 0.0 and hs[2] != 0.0 and abs(hs[3]) > 1e-3:
                quiet = [int(c) + 1 for c in order[::-1] if abs(b[c]) < 0.5 * lam and c not in (j, k)]
                return j + 1, k + 1, lam, quiet
    raise AssertionError("no such pair")


@pytest.mark.parametrize("lane", [1, 2, 63, 64])
def test_repeat_of_a_stored_zero_that_moves_later(list_handle, lane):
    """[k, quiet..., k, j, k] with k's repeat at `lane`: both first visits of k settle (one stored zero), j moves, and then k
    moves to a non-zero, so dropzeros! keeps its slot.  A chunk that took k and its repeat together would store k twice, and
    both slots would survive: the support would name k twice.  Lane 64 opens the next chunk (no repeat inside either chunk)."""
    f = list_handle
    b = _list_problem()[0]
    j, k, lam, quiet = _repeat_case()
    lst = [k] + quiet[: lane - 1] + [k, j, k]
    assert lst.index(k, 1) == lane and len(set(lst)) == len(lst) - 2
    g, go = cd.ProxL1(lam), O.ProxL1(lam)
    fo, fc = O.CDQuadraticLoss(_A(P_L), b), O.CDQuadraticLoss(_A(P_L), b)
    x, xo = _pair(P_L, [])
    cd.initialize_(f, x)
    O.initialize_(fo, xo)
    xc = O.SparseIterate(P_L)                                # the oracle's own account of the visits, one by one
    hs = [O.descendCoordinate_(fc, go, xc, c) for c in lst]
    assert not any(hs[:-2]) and hs[-2] != 0.0 and hs[-1] != 0.0
    assert xc.nnz == len(lst) - 2 and xc.nzval2ind.tolist()[0] == k          # every settled visit stored a zero, k once
    mh, mho = cd.cdPass_(x, f, g, lst), O.cdPass_(xo, fo, go, lst)
    assert abs(mh - mho) <= H_TOL and mho == max(abs(hs[-2]), abs(hs[-1]))
    assert sorted(xo.nzval2ind.tolist()) == sorted([j, k])
    assert x.nnz == 2 and x.nzval2ind.tolist() == xo.nzval2ind.tolist()
    np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL)
    np.testing.assert_allclose(f._gradient_vector(0), _oracle_gradient(fo), rtol=0, atol=_grad_bar(b))
    _grad_check(f, 0, x, b)


@pytest.mark.parametrize("how", ["pass", "descend", "solve"])
def test_infinite_omega_empties_a_stored_coordinate(list_handle, how):
    f = list_handle
    b, entries = _list_problem()
    fo = O.CDQuadraticLoss(_A(P_L), b)
    x, xo = _pair(P_L, entries)
    k0, v0 = entries[3]
    om = np.ones(P_L)
    om[k0 - 1] = np.inf
    lam = 0.3 * float(np.abs(b).max())
    g, go = cd.ProxL1(lam, om), O.ProxL1(lam, om)
    if how == "solve":
        o = dict(OPT, warmStart=True, randomize=False)
        cd.coordinateDescent_(x, f, g, cd.CDOptions(**o))
        st = O.coordinateDescent_(xo, fo, go, O.CDOptions(**o))
        assert st["converged"]
        _same(f.last_stats, x, st, xo)
    else:
        cd.initialize_(f, x)
        O.initialize_(fo, xo)
        if how == "descend":
            h, ho = cd.descendCoordinate_(f, g, x, k0), O.descendCoordinate_(fo, go, xo, k0)
            assert h == ho == -v0
            assert x.nzval2ind.tolist() == xo.nzval2ind.tolist() and k0 in x.nzval2ind.tolist()    # a stored zero until a pass ends
        lst = [k0] + [k for k, _ in entries[:40]]
        mh, mho = cd.cdPass_(x, f, g, lst), O.cdPass_(xo, fo, go, lst)
        assert abs(mh - mho) <= H_TOL and (how == "descend" or mho >= abs(v0))
        np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL)
        assert x.nzval2ind.tolist() == xo.nzval2ind.tolist()
    assert x[k0] == 0.0 and k0 not in x.nzval2ind.tolist() and x.nnz > 0
    _grad_check(f, 0, x, b)


# ---- 6. non-finite input stays in its own problem -----------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["b", "start"])
@pytest.mark.parametrize("rand", [False, True], ids=["ordered", "shuffled"])
def test_nan_stays_in_its_problem(rand, where):
    """Problem 1 of 3 holds one NaN: in b (S(NaN, t) = 0 on both sides: the visit of that coordinate stores a zero and moves
    nothing, only g carries the NaN), or in its start (x_k = NaN: h = NaN moves, the whole gradient becomes NaN, |h| = NaN never
    raises maxH; coordinate_descent.jl:104, cd_differentiable_function.jl:333-337).  maxIter = 20; problems 0 and 2 converge
    within it, problem 1 is held to whatever the oracle does."""
    p, m = 65, 3
    A = _A(p)
    rng = np.random.default_rng(60 + rand)
    B = np.stack([_b(p, 950 + j, s=3) for j in range(m)], axis=1)
    lams = [0.5 * float(np.abs(B[:, j]).max()) for j in range(m)]
    starts = [_entries(rng, p, n) for n in (5, 9, 7)]
    Bn, startn = B.copy(), list(starts)
    if where == "b":
        Bn[7, 1] = np.nan
    else:
        startn[1] = starts[1][:4] + [(starts[1][4][0], float("nan"))] + starts[1][5:]
    opts = dict(maxIter=20, optTol=1e-12, warmStart=True, randomize=rand, seed=3)
    pens = [cd.ProxL1(l) for l in lams]
    clean, dirty = cd.CDQuadraticLoss(A, B), cd.CDQuadraticLoss(A, Bn)
    xc = [_pair(p, e)[0] for e in starts]
    pairs = [_pair(p, e) for e in startn]
    xd = [x for x, _ in pairs]
    cd.coordinateDescent_(xc, clean, pens, cd.CDOptions(**opts))
    cd.coordinateDescent_(xd, dirty, pens, cd.CDOptions(**opts))
    for j in (0, 2):
        assert _bits(xd[j]) == _bits(xc[j]) and dirty.last_stats[j] == clean.last_stats[j], j
        assert dirty._gradient_vector(j).tobytes() == clean._gradient_vector(j).tobytes(), j
    for j in range(m):
        fo, xo = O.CDQuadraticLoss(A, Bn[:, j].copy()), pairs[j][1]
        st = O.coordinateDescent_(xo, fo, O.ProxL1(lams[j]), O.CDOptions(**opts))
        assert j == 1 or st["converged"]
        assert np.array_equal(np.isnan(xd[j].dense()), np.isnan(xo.dense())), j
        _same(dirty.last_stats[j], xd[j], st, xo, tag=j)     # (assert_allclose: NaN in the same places, the rest within 1e-10)
        go = _oracle_gradient(fo)
        assert np.array_equal(np.isnan(dirty._gradient_vector(j)), np.isnan(go)), j
    assert np.isnan(dirty._gradient_vector(1)).any()
    if where == "start":
        assert np.isnan(dirty._gradient_vector(1)).all()     # the NaN step did move: g += NaN A[:, k]
    clean.close()
    dirty.close()


# ---- 7. sequences on one handle ----------------------------------------------------------------------------------------------
from _quad_sequences import MAXB, P_S, _run_sequence  # noqa: E402


@pytest.mark.parametrize("seed", range(30))
def test_sequence_on_one_handle(seed):
    assert 12 <= len(_run_sequence(seed)) <= 15


def test_set_b_smaller_then_larger():
    """m = 5 -> 2 -> 6 on one handle: a new b is a new loss, whatever the problems beyond the smaller m held before."""
    A = _A(P_S)
    rng = np.random.default_rng(71)
    f = None
    for step, m in enumerate((5, 2, 6)):
        B = np.stack([_b(P_S, 1000 + 10 * step + j, s=2 + j) for j in range(m)], axis=1)
        if f is None:
            f = cd.CDQuadraticLoss(A, B, max_batch=MAXB)
        else:
            f.set_b(B)
        for j in range(m):                                   # as a new loss: the iterate zero, A x = 0
            assert _raw_state(f, j) == (b"", b"", B[:, j].tobytes())
        lams = [(0.05 + 0.03 * j) * float(np.abs(B[:, j]).max()) for j in range(m)]
        opts = dict(OPT, warmStart=True, randomize=True, seed=step)
        pairs = [_pair(P_S, e) for e in ([[]] * m if step == 2 else _batch_starts(rng, P_S, m))]
        xs = [x for x, _ in pairs]
        cd.coordinateDescent_(xs, f, [cd.ProxL1(l) for l in lams], cd.CDOptions(**opts))
        for j in range(m):
            fo, xo = O.CDQuadraticLoss(A, B[:, j].copy()), pairs[j][1]
            st = O.coordinateDescent_(xo, fo, O.ProxL1(lams[j]), O.CDOptions(**opts))
            assert st["converged"] and xo.nnz > 0
            _same(f.last_stats[j], xs[j], st, xo, tag=(m, j))
            _grad_check(f, j, xs[j], B[:, j], tag=(m, j))
    f.close()


def test_raw_refusals_after_set_b():
    L, BAD = cd._lib.lib(), cd._lib.CDH_BAD_ARG
    B = np.stack([_b(P_S, 1100 + j) for j in range(4)], axis=1)
    f = cd.CDQuadraticLoss(_A(P_S), B, max_batch=MAXB)
    xs = [cd.SparseIterate(P_S) for _ in range(4)]
    cd.coordinateDescent_(xs, f, cd.ProxL1(0.3 * float(np.abs(B).max())), cd.CDOptions(**OPT))     # (the handle has a penalty)
    B2 = np.asfortranarray(B[:, :2])
    assert L.cdh_quad_set_b(f._h, 2, _vp(B2), P_S) == cd._lib.CDH_OK
    o, st, out = cd.CDOptions(**OPT)._c(), (cd._lib.cdh_stats * 2)(), C.c_double()
    one = np.array([1], dtype=np.int64)
    for rc in (L.cdh_quad_coordinate_descent(f._h, C.byref(o), st), L.cdh_quad_descend(f._h, 0, 1, C.byref(out)),
               L.cdh_quad_pass(f._h, 0, 1, _vp(one), C.byref(out))):
        assert rc == BAD
        assert b"cdh_quad_set_penalty has not been called since cdh_quad_set_b" in L.cdh_last_error(None)
    nnz, idx, val = C.c_int64(), np.zeros(P_S, dtype=np.int64), np.zeros(P_S)
    assert L.cdh_quad_get_iterate(f._h, 2, C.byref(nnz), _vp(idx), _vp(val)) == BAD                  # j = m: a problem of the old b
    assert b"problem index j outside 0 .. m - 1" in L.cdh_last_error(None)
    assert L.cdh_quad_get_gradient(f._h, 2, _vp(val)) == BAD
    assert L.cdh_quad_get_iterate(f._h, 1, C.byref(nnz), _vp(idx), _vp(val)) == cd._lib.CDH_OK and nnz.value == 0
    lam = np.array([0.2, 0.3])
    assert L.cdh_quad_set_penalty(f._h, _vp(lam), None, 0) == cd._lib.CDH_OK
    assert L.cdh_quad_coordinate_descent(f._h, C.byref(o), st) == cd._lib.CDH_OK
    f.close()
