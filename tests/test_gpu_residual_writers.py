"""The kernels that WRITE the residual r = y - X beta in place, checked row by row: k_init_resid (initialize!, and the lazy
rebuild after a one-launch solve), k_step / k_axpy (the per-coordinate sweep), k_blockstep<B <= 8> / k_block_axpy, phase A
of every k_gramstep<T, NG, LT, KS> instantiation, and k_multi_axpy for both of its callers (the trailing update of a
wide-block pass; sync_r's catch-up after cache-served solves).  test_gpu_kernel_sums.py checks the kernels that read rows
and sum them; a row -- or a whole chunk of rows -- that misses one update among 10^7 passes every check of sums.

Two oracles.

(a) k_init_resid on integer X, y and beta: every product and partial sum is an integer below 2^53 (2^24 once stored as
fp32), asserted below, so r must equal numpy's y - X beta bit for bit.

(b) Everywhere else the moves are not exact numbers, so the test takes the beta the GPU itself reports and checks EVERY row
against r_ref = y - X beta_gpu accumulated in numpy.longdouble (64-bit significand: each of its at most 2 m operations per
row errs by 2^-64 of the partial sum, three orders of magnitude below the bound).  X is integer-valued in {+-1, +-2, +-3}
with no zero entry, y integer-valued and non-zero.  The bound for row i:

    |r_gpu[i] - r_ref[i]| <= 2 (M 2^-53 + L u_T) A_i ,      A_i = |y_i| + sum_k |x_ik| TV_k

    M    non-zero moves applied since r was last exact (r = y at beta = 0; an initialize! at beta != 0 counts its nnz
         fmas and its subtraction: nnz + 1)
    L    launches that stored r since then: m for the per-coordinate sweep, ceil(m / B) + 1 for the blocked ones (one more
         than store: the first launch of a pass has nothing to apply), 1 per initialize!, 1 per batch of 64 of sync_r
    u_T  unit roundoff of the storage type: 2^-53 (fp64), 2^-24 (fp32)
    TV_k total variation of beta_k since r was last exact: |beta_after - beta_before| per pass without a repeated
         coordinate; from a visit-by-visit fp64 replay for the list that repeats one

Derivation.  Every kernel keeps the row in fp64 registers through a launch, applies each move as one fma
(re = fma(-h, x, re)) and rounds to T once when it stores.  Every intermediate value of row i is a partial sum of
y_i - sum x_ik h, bounded by A_i (to first order).  Write S for the launches that really store r (S = L, except in the
blocked modes, where the formula above over-counts by the first launch of the pass: S = L - 1).  The M fmas err by at most
M 2^-53 A_i and the stores by S u_T A_i.  The short-chunk k_gramstep variants alone add the partial sums of their 2 or 4
column groups with a butterfly: at most 2 more fp64 roundings per storing launch, 2 S 2^-53 A_i.  And r is driven by
h = fl(new - old) while the reference uses beta itself: sum_k |x_ik| 2^-53 TV_k <= 2^-53 A_i in all.  Total

    (M + 2 S + 1) 2^-53 A_i + S u_T A_i     (2 S only with the butterfly)     against     2 M 2^-53 A_i + 2 L u_T A_i .

fp32 storage: S u_T <= L u_T leaves L 2^-24 for (2 S + 1) 2^-53: always.  fp64 storage: M + 3 S + 1 <= 2 M + 2 L, that is
3 S + 1 <= M + 2 L; with S = L - 1 (every butterfly case is a blocked mode) that is L <= M + 2, and a blocked pass has
L = ceil(m / B) + 1 <= M + 1 whenever each of its blocks holds a move (asserted by the cases).  Without the butterfly M + S + 1 <= 2 M + 2 L holds for any
M >= 1.  Nothing in the bound is measured; test_bound_holds_for_the_cpu_replay replays the recipe in numpy (no GPU) at the largest M and L any
case here uses (MAX_M, MAX_L, asserted by every case) and checks that it stays inside.

Detectability.  A move is DETECTABLE when |h| min|x| = |h| exceeds 100 x the largest bound of its case: one dropped or
doubled (row, move) pair is then outside the bound by two orders of magnitude.  Every case asserts the branch it is named
for counting detectable moves only (the variant chosen, the wraps of the chunk loop, nzp, the rounds of PG * CGN, the
batches of 64), and that every launch that stores r applies at least one.  The data keeps A_i small so that this holds for
fp32 storage too: planted coefficients of 0.5 .. 1.5 on the coordinates that are meant to move, lambda = 0 for them and an
infinite-looking penalty weight for those that are meant to stay (h = 0 exactly: the holes of the ballot compaction).

Shapes are computed from the device's CU count with the Python twin of the host's grid and variant policy (tests/_sweep_plan.py,
held to csrc/sweep_plan.hpp on the CPU by tests/test_sweep_plan_host.py).  Knobs are read when a handle is made: they are set before the loss is constructed.
"""
import zlib

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
from coordinatedescent_jl_amd._lib import check
# cus: the CU-count fixture.  It asks torch, and torch finds the device only if it initialises before the library has opened
# it in this process (two HIP runtimes are loaded, torch's own and the library's; the library exports no CU count), so EVERY
# GPU test here requests it, whether it sizes a shape from it or not.
from test_gpu_kernel_sums import U64, _ints, _int_y, _nv, _vp, cus  # noqa: F401
from test_gpu_kernel_sums import F32_XMAX, F32_YMAX, F64_XMAX, F64_YMAX
# the grids and the wide-block variant policy: the twin of csrc/sweep_plan.hpp
from _sweep_plan import block_grid, gram_launch, init_grid, step_grid
from _sweep_plan import nvec as _nvec

gpu = pytest.mark.gpu
U32 = 2.0 ** -24
DETECT = 100.0
MAX_M, MAX_L = 210, 70                 # no case below goes beyond these counts (asserted in _check); the CPU replay reaches them
assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended-precision long double"

DTYPES = [np.float64, np.float32]
DT_IDS = ["float64", "float32"]


def _ut(dtype):
    return U64 if dtype == np.float64 else U32


KNOBS = {"default": {}, "frag": {"CDH_LT": "0"}, "lt_long": {"CDH_LT": "1", "CDH_KS": "2"},
         "lt_short": {"CDH_LT": "1", "CDH_KS": "1"}}


def _knob_args(name):
    k = KNOBS[name]
    return {"lt": int(k.get("CDH_LT", 2)), "ks": int(k.get("CDH_KS", 0))}


def _set_knobs(monkeypatch, name):
    for k in ("CDH_LT", "CDH_KS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in KNOBS[name].items():
        monkeypatch.setenv(k, v)


# ---- data ---------------------------------------------------------------------------------------------------------------
_LUT = np.array([-3, -2, -1, 1, 2, 3], dtype=np.int8)


def _data(seed, n, p, dtype, planted, tie=None):
    """X8: p x n int8 in {+-1, +-2, +-3} (its transpose is the Fortran-order X); y = rint(X beta*), zeros replaced by 1,
    beta* of magnitude 0.5 .. 1.5 on the 0-based coordinates `planted`.  Everything is exact in fp32 as well.  tie = (a, b):
    column b copies column a on the first half of the rows, so that a second visit of a after b moves by about h_b / 2."""
    rng = np.random.default_rng(seed)
    X8 = _LUT[rng.integers(0, 6, size=(p, n), dtype=np.int8)]
    if tie is not None:
        X8[tie[1], :n // 2] = X8[tie[0], :n // 2]
    bstar = rng.uniform(0.5, 1.5, size=len(planted)) * rng.choice([-1.0, 1.0], size=len(planted))
    y = np.zeros(n)
    for k, b in zip(planted, bstar):
        y += X8[k] * b
    y = np.rint(y)
    y[y == 0] = 1.0
    assert np.abs(y).max() + 3 * 1.5 * len(planted) < 2 ** 24
    return X8, y.astype(dtype), rng


def _make_loss(kind, dtype, X8, y, w=None):
    """The loss for X = X8' in `dtype`.  Small matrices through the constructor; large ones are uploaded in column batches
    from the int8 copy, so that the host never holds the matrix in working precision."""
    p, n = X8.shape
    cls = {"ls": cd.CDLeastSquaresLoss, "sqrt": cd.CDSqrtLassoLoss, "wls": cd.CDWeightedLSLoss}[kind]
    isz = np.dtype(dtype).itemsize
    if n * p * isz <= (256 << 20):
        X = X8.T.astype(dtype)                          # Fortran order, kept by astype
        return cls(y, X, w) if kind == "wls" else cls(y, X)
    f = cls.__new__(cls)
    f._create(np.dtype(dtype), n, p, 0, None, 0)
    step = max(1, (64 << 20) // (n * isz))
    for j0 in range(0, p, step):
        blk = np.asfortranarray(X8[j0:j0 + step].T.astype(dtype))
        check(f._L.cdh_set_X_cols(f._h, j0, blk.shape[1], _vp(blk), n), f._h)
    check(f._L.cdh_set_y(f._h, _vp(np.ascontiguousarray(y))), f._h)
    if w is not None:
        check(f._L.cdh_set_obs_weights(f._h, _vp(np.ascontiguousarray(w, dtype=dtype))), f._h)
    return f


def _ref_and_scale(X8, y, beta, TV):
    """(y - X beta in long double, A_i = |y_i| + sum_k |x_ik| TV_k), column by column from the int8 copy."""
    ref = y.astype(np.longdouble)
    A = np.abs(y.astype(np.float64))
    for k in np.nonzero((beta != 0.0) | (TV != 0.0))[0]:
        if beta[k] != 0.0:
            ref -= X8[k].astype(np.longdouble) * np.longdouble(beta[k])
        A += np.abs(X8[k]).astype(np.float64) * TV[k]
    return ref, A


def _check(what, X8, y, dtype, r_gpu, beta, TV, M, L):
    """Every row of r_gpu within the bound; returns the largest bound of the case."""
    assert 0 < M <= MAX_M and 0 < L <= MAX_L, (what, M, L)
    ref, A = _ref_and_scale(X8, y, beta, TV)
    bound = 2.0 * (M * U64 + L * _ut(dtype)) * A
    err = np.abs(r_gpu.astype(np.longdouble) - ref).astype(np.float64)
    ratio = float(np.max(err / bound))
    print(f"{what}: n={y.shape[0]} M={M} L={L} max err/bound={ratio:.3g} max bound={bound.max():.3g}")
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, (what, f"{bad.size} rows outside the bound", bad[:8].tolist(), bad[-4:].tolist(),
                           (err[bad[:8]] / bound[bad[:8]]).tolist())
    return float(bound.max())


def _replay_ls(X8, y, visit1):
    """The visit-by-visit moves of a least-squares pass at lambda = 0 from beta = 0, in fp64 (for a list that repeats a
    coordinate: the GPU reports one value per coordinate, the total variation needs every visit)."""
    r, hs, beta = y.astype(np.float64).copy(), [], np.zeros(X8.shape[0])
    for k1 in visit1:
        xk = X8[k1 - 1].astype(np.float64)
        h = float(xk @ r) / float(xk @ xk)
        r -= h * xk
        beta[k1 - 1] += h
        hs.append(h)
    return np.array(hs), beta


def _run_pass(what, f, X8, y, dtype, mode, visit1, movers=None, sqrt=False):
    """initialize! at beta = 0 (r = y, exact), one cdPass_ over the 1-based list `visit1` in sweep mode `mode` ("coord" or
    the block width), every row of f.r checked.  movers: 0-based coordinates allowed to move (the others carry a penalty
    weight that keeps them at zero); None: all, lambda = 0.  Returns (h per visit position, detectable per position)."""
    p = X8.shape[0]
    visit1 = np.ascontiguousarray(visit1, dtype=np.int64)
    m = len(visit1)
    f.set_screening(False)
    f.set_gradient_cache(0)
    if mode == "coord":
        f.set_sweep_mode("coord")
    else:
        f.set_sweep_mode("block", mode)
    if movers is None:
        g = cd.ProxL1(0.0)
    else:
        om = np.full(p, 1e30)
        om[list(movers)] = 0.0
        g = cd.ProxL1(1.0, om)
    x = cd.SparseIterate(p)
    cd.initialize_(f, x)
    np.testing.assert_array_equal(f.r, y)
    st0 = f.cache_stats()
    cd.cdPass_(x, f, g, visit1)
    assert f.cache_stats()["covariance_visits"] == st0["covariance_visits"] == 0       # the streamed kernels ran
    beta = x.dense()
    dup = len(set(visit1.tolist())) < m
    if dup:
        assert movers is None and not sqrt
        h, beta_replay = _replay_ls(X8, y, visit1)
        np.testing.assert_allclose(beta, beta_replay, rtol=0, atol=1e-9 if dtype == np.float64 else 1e-4)
        TV = np.zeros(p)
        np.add.at(TV, visit1 - 1, np.abs(h) * (1.0 + 1e-3))
    else:
        h, TV = beta[visit1 - 1], np.abs(beta)
    M = int(np.count_nonzero(h))
    L = m if mode == "coord" else -(-m // mode) + 1
    bmax = _check(what, X8, y, dtype, f.r, beta, TV, M, L)
    det = np.abs(h) > DETECT * bmax
    if movers is not None:
        stay = ~np.isin(visit1 - 1, list(movers))
        assert np.all(h[stay] == 0.0), what                         # the holes are exact zeros
    return h, det


def _blocks(det, B):
    """Detectable moves per launch of a blocked pass: block b's moves are applied by launch b + 1 (the trailing axpy last)."""
    return [int(det[i:i + B].sum()) for i in range(0, len(det), B)]


# ---- the bound itself, on the CPU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["coord", 8, 64])
def test_bound_holds_for_the_cpu_replay(dtype, mode):
    """No GPU: the kernels' recipe in numpy -- sequential fp64 updates of r (a multiply and a subtraction each: one rounding
    more than the kernels' fma), one rounding to T per launch -- run until M and L reach the largest counts any GPU case
    uses, stays within the bound of the long-double reference.  If it does not, the bound's constant is wrong."""
    n, p = 4099, 70
    X8, y, _ = _data(1, n, p, dtype, list(range(p)))
    r, beta, TV, M, L = y.astype(np.float64).copy(), np.zeros(p), np.zeros(p), 0, 0
    B = 1 if mode == "coord" else mode
    worst = 0.0
    while M + p <= MAX_M and L + (p if mode == "coord" else -(-p // B) + 1) <= MAX_L:
        for b0 in range(0, p, B):
            ks = range(b0, min(p, b0 + B))
            hs, rb = [], r.copy()                         # the block's moves from the Gram recurrence = sequential on r
            for k in ks:
                xk = X8[k].astype(np.float64)
                h = float(xk @ rb) / float(xk @ xk)
                rb -= h * xk
                hs.append(h)
            for k, h in zip(ks, hs):                      # applied by the next launch, stored once
                r -= h * X8[k].astype(np.float64)
                new = beta[k] + h
                TV[k] += abs(new - beta[k])
                beta[k] = new
                M += 1
            r = r.astype(dtype).astype(np.float64)
            L += 1
        L += 0 if mode == "coord" else 1
        ref, A = _ref_and_scale(X8, y, beta, TV)
        bound = 2.0 * (M * U64 + L * _ut(dtype)) * A
        err = np.abs(r.astype(np.longdouble) - ref).astype(np.float64)
        assert np.all(err <= bound), (M, L, float(np.max(err / bound)))
        worst = max(worst, float(np.max(err / bound)))
    assert (L == MAX_L) if mode == "coord" else (M == MAX_M), (M, L)
    print(f"cpu replay {np.dtype(dtype).name} {mode}: M={M} L={L} max err/bound={worst:.3g}")


# ---- (a) k_init_resid, bit for bit ---------------------------------------------------------------------------------------
F64_BMAX, F32_BMAX, INIT_NNZ_MAX = 1 << 20, 500, 200
assert F64_YMAX + INIT_NNZ_MAX * F64_XMAX * F64_BMAX < 2 ** 53            # |y| + sum |x| |beta|: every partial sum exact
assert F32_YMAX + INIT_NNZ_MAX * F32_XMAX * F32_BMAX < 2 ** 24            # ... and the result exact in fp32 storage


def _init_shapes(dtype):
    nv = _nv(dtype)
    small = [1, max(1, nv - 1), 255 * nv, 256 * nv, 256 * nv + 1, 5003]
    return [(n, 210, nnz) for n in dict.fromkeys(small) for nnz in (1, 3, 64, 65, 200)] + \
           [(2048 * 256 * nv + 3 * nv + 1, 4, nnz) for nnz in (1, 3)]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_init_resid_is_exact_on_integer_data(cus, dtype):
    """initialize!(f, x) with an integer iterate whose support is in no particular order (a SparseIterate repeats no
    coordinate): f.r equals y - X beta exactly, at the tails of the 256-vector block, with a support longer than any
    unroll, and past the 2048-block cap of the grid (every block walks a second stride)."""
    bmax = F64_BMAX if dtype == np.float64 else F32_BMAX
    for n, p, nnz in _init_shapes(dtype):
        if n > 5003:
            assert _nvec(n, dtype) > init_grid(n, dtype) * 256 and init_grid(n, dtype) == 2048
        rng = np.random.default_rng(n * 7 + nnz)
        X, y = _ints(rng, n, p, dtype), _int_y(rng, n, dtype)
        f = cd.CDLeastSquaresLoss(y, X)
        sup = rng.permutation(p)[:nnz]
        if nnz > 2:
            sup[:3] = np.sort(sup[:3])[::-1]                   # descending somewhere: not ascending order
            assert np.any(np.diff(sup) < 0)
        assert len(set(sup.tolist())) == nnz
        vals = rng.integers(1, bmax + 1, size=nnz) * rng.choice([-1, 1], size=nnz)
        x = cd.SparseIterate(p)
        for k, v in zip(sup, vals):
            x[int(k) + 1] = float(v)
        assert x.nzval2ind.tolist() == (sup + 1).tolist()
        cd.initialize_(f, x)
        X64 = X[:, sup].astype(np.float64)
        want = y.astype(np.float64) - X64 @ vals.astype(np.float64)
        assert np.abs(y.astype(np.float64)).max() + (np.abs(X64) @ np.abs(vals.astype(np.float64))).max() < \
            (2 ** 53 if dtype == np.float64 else 2 ** 24)
        np.testing.assert_array_equal(f.r, want.astype(dtype), err_msg=f"n={n} nnz={nnz}")
        f.close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_lazy_rebuild_after_a_one_launch_solve(monkeypatch, cus, dtype):
    """The one-launch solve leaves r stale; reading f.r rebuilds it (sync_r -> rebuild_residual_from(the lazy iterate): one
    k_init_resid launch with a non-integer iterate): M = nnz + 1 operations, one store, TV = |beta|."""
    monkeypatch.setenv("CDH_SMALL_PATH", "1")
    n, p, s = 1003, 50, 12
    X8, y, _ = _data(21, n, p, dtype, list(range(0, 2 * s, 2)))
    f = _make_loss("ls", dtype, X8, y)
    x = cd.SparseIterate(p)
    cd.coordinateDescent_(x, f, cd.ProxL1(0.5), cd.CDOptions(maxIter=200, optTol=1e-9, randomize=False))
    assert f.onchip_stats()["solves"] == 1 and x.nnz >= s
    beta = x.dense()
    bmax = _check("lazy rebuild", X8, y, dtype, f.r, beta, np.abs(beta), x.nnz + 1, 1)
    assert int((np.abs(beta) > DETECT * bmax).sum()) >= s
    f.close()


# ---- 1. tails and wrap-around, per writer ---------------------------------------------------------------------------------
def _tail_sizes(units, dtype):
    nv = _nv(dtype)
    out = [1, max(1, nv - 1)]
    for u in units:
        out += [(u - 1) * nv, u * nv, u * nv + 1]       # one vector short of the unit, at it, one (partial) vector past it
    return list(dict.fromkeys(out))


def _visits_for(n, pfull):
    """All-move lists need rows to spare: r is (nearly) zero once n coordinates have moved, and later visits move nothing."""
    return max(1, min(pfull, n // 8))


TAIL_CASES = ([(d, l, "coord") for d in DTYPES for l in ("ls", "wls")] + [(np.float64, "sqrt", "coord")]
              + [(d, "ls", B) for d in DTYPES for B in (2, 4, 8)] + [(np.float32, "sqrt", 8)]
              + [(d, l, B) for d in DTYPES for l in ("ls", "wls") for B in (16, 32, 64)] + [(np.float64, "sqrt", 64)])


@gpu
@pytest.mark.parametrize("dtype,loss,mode", TAIL_CASES, ids=[f"{np.dtype(d).name}-{l}-{m}" for d, l, m in TAIL_CASES])
def test_tails_of_every_writer(monkeypatch, cus, dtype, loss, mode):
    """n = 1, NV - 1, and one vector short of / at / one row past each unit of the writer: the 1024-vector tile of k_step /
    k_axpy, the 256-vector stride of k_blockstep / k_block_axpy / k_multi_axpy, the chunk length CVN of each k_gramstep
    variant (default policy and pinned).  The last row is checked like every other."""
    wide = mode != "coord" and mode >= 16
    knob_sets = ["default", "frag", "lt_long", "lt_short"] if wide else ["default"]
    if wide and dtype == np.float32 and mode == 64:
        knob_sets = ["default"]                           # fp32 B = 64 has the fragment variant only
    for knobs in knob_sets:
        _set_knobs(monkeypatch, knobs)
        if mode == "coord":
            units, pfull = [1024], 7
        elif not wide:
            units, pfull = [256], mode + 3
        else:
            units, pfull = [256], mode + 6
        for n in _tail_sizes(units + ([16, 32, 64] if wide else []), dtype):
            m = _visits_for(n, pfull)
            what = f"tail {np.dtype(dtype).name} {loss} {mode} {knobs} n={n} m={m}"
            if wide:
                gl = gram_launch(n, dtype, mode, cus, **_knob_args(knobs))
                assert gl["rounds"] == 1 and (knobs == "default" or gl["variant"] == knobs or
                                              (mode == 16 and knobs == "lt_short" and gl["variant"] == "lt_long")), (what, gl)
            X8, y, rng = _data(zlib.crc32(what.encode()), n, pfull, dtype, list(range(m)))
            w = rng.integers(1, 4, size=n).astype(dtype) if loss == "wls" else None
            f = _make_loss(loss, dtype, X8, y, w)
            h, det = _run_pass(what, f, X8, y, dtype, mode, np.arange(1, m + 1), sqrt=loss == "sqrt")
            assert det[0], (what, h)                      # the first launch that stores applies a detectable move
            if wide:
                assert all(c >= 1 for c in _blocks(det, mode)), (what, h)      # every storing launch applies one
            elif n >= 8 * pfull:
                assert det.all(), (what, h)
            f.close()


WRAP_CASES = ([(d, l, "coord") for d, l in ((np.float64, "ls"), (np.float64, "wls"), (np.float32, "ls"))]
              + [(d, "ls", B) for d in DTYPES for B in (2, 4, 8)] + [(np.float64, "sqrt", 8), (np.float32, "sqrt", 4)])
# (no weighted-LS row for B <= 8: k_blockstep takes no observation weights, and run_chunk sends a weighted loss with a narrow
# block to k_step -- the "coord" rows above)


@gpu
@pytest.mark.parametrize("dtype,loss,mode", WRAP_CASES, ids=[f"{np.dtype(d).name}-{l}-{m}" for d, l, m in WRAP_CASES])
def test_grid_stride_wraps_of_the_vector_alu_writers(cus, dtype, loss, mode):
    """Past step_grid tiles of 1024 vectors (k_step, k_axpy) and past block_grid strides of 256 (k_blockstep, k_block_axpy):
    every block goes round its loop a second time, the last ones do not.  All-move and half-move lists, m not a multiple
    of B, the last block ragged."""
    nv = _nv(dtype)
    if mode == "coord":
        n, p = (min(2048, 8 * cus) * 1024 + 1024 + 3) * nv - 1, 5
        assert _nvec(n, dtype) > step_grid(n, dtype, cus) * 1024 and step_grid(n, dtype, cus) == min(2048, 8 * cus)
    else:
        n, p = (3 * cus * 256 + 256 + 3) * nv - 1, mode + 3
        assert _nvec(n, dtype) > block_grid(n, dtype, cus) * 256 and block_grid(n, dtype, cus) == 3 * cus and p % mode != 0
    what = f"wrap {np.dtype(dtype).name} {loss} {mode}"
    X8, y, rng = _data(zlib.crc32(what.encode()), n, p, dtype, list(range(p)))
    w = rng.integers(1, 4, size=n).astype(dtype) if loss == "wls" else None
    f = _make_loss(loss, dtype, X8, y, w)
    h, det = _run_pass(what + " all-move", f, X8, y, dtype, mode, np.arange(1, p + 1), sqrt=loss == "sqrt")
    assert det.all(), (what, h)
    movers = list(range(0, p, 2))
    h, det = _run_pass(what + " half-move", f, X8, y, dtype, mode, np.arange(1, p + 1), movers=movers, sqrt=loss == "sqrt")
    assert det[movers].all() and det.sum() == len(movers), (what, h)
    if mode != "coord":
        assert all(c >= 1 for c in _blocks(det, mode))
    f.close()


def _first_wrap_n(dtype, B, cus, knobs, extra_vectors):
    """Rows for exactly Gmax * kGramWaves chunks of the variant's length (+ extra_vectors more vectors)."""
    nv = _nv(dtype)
    gl = gram_launch(1 << 20, dtype, B, cus, **_knob_args(knobs))        # (any mid size: Gmax and, pinned, CVN do not move)
    cvn = gl["CVN"]
    for _ in range(3):                                                     # the default policy's CVN depends on n: settle
        n = (cvn * 4 * gl["Gmax"] + extra_vectors) * nv
        g2 = gram_launch(n, dtype, B, cus, **_knob_args(knobs))
        if g2["CVN"] == cvn and g2["Gmax"] == gl["Gmax"]:
            return n, g2
        cvn, gl = g2["CVN"], g2
    raise AssertionError(("no consistent size", np.dtype(dtype).name, B, knobs))


FIRST_WRAP = [(d, B, k) for d in DTYPES for B in (16, 32, 64) for k in ("default", "frag", "lt_long", "lt_short")
              if not (d == np.float32 and B == 64 and k in ("lt_long", "lt_short")) and not (B == 16 and k == "lt_short")]


@gpu
@pytest.mark.parametrize("dtype,B,knobs", FIRST_WRAP, ids=[f"{np.dtype(d).name}-{B}-{k}" for d, B, k in FIRST_WRAP])
def test_first_wrap_of_the_chunk_loop(monkeypatch, cus, dtype, B, knobs):
    """Exactly G * kGramWaves chunks (no wave goes round twice), and one vector more (wave 0 of block 0 does)."""
    _set_knobs(monkeypatch, knobs)
    p = B + 6
    for extra, rounds in ((0, 1), (1, 2)):
        n, gl = _first_wrap_n(dtype, B, cus, knobs, extra)
        assert gl["G"] == gl["Gmax"] and gl["rounds"] == rounds and gl["nchunks"] == 4 * gl["G"] + extra, gl
        assert knobs == "default" or gl["variant"] == knobs
        what = f"first wrap {np.dtype(dtype).name} B={B} {knobs} {gl['variant']} +{extra}"
        X8, y, _ = _data(zlib.crc32(what.encode()), n, p, dtype, list(range(p)))
        f = _make_loss("ls", dtype, X8, y)
        h, det = _run_pass(what, f, X8, y, dtype, B, np.arange(1, p + 1))
        assert det.all() and _blocks(det, B) == [B, 6], (what, h)
        f.close()


# ---- 2. every k_gramstep variant: pinned at a mid size, and by the default policy ------------------------------------------
PINNED = ([(d, "ls", k) for d in DTYPES for k in ("frag", "lt_long", "lt_short")]
          + [(np.float64, "wls", "lt_long"), (np.float32, "wls", "frag"), (np.float64, "sqrt", "lt_short")])


@gpu
@pytest.mark.parametrize("dtype,loss,knobs", PINNED, ids=[f"{np.dtype(d).name}-{l}-{k}" for d, l, k in PINNED])
def test_pinned_variants_where_the_chunk_loop_wraps_twice(monkeypatch, cus, dtype, loss, knobs):
    """CDH_LT / CDH_KS pin the variant; n is such that every wave of every variant goes round its chunk loop at least
    three times (two wraps), with a ragged last vector.  All-move blocks: nzp = B, several rounds of PG * CGN previous
    columns; a full block after a full block (nprev = nb = B: p = 70 is 32 + 32 + 6 and 4 x 16 + 6) and nprev = 6 < B on the
    last one."""
    _set_knobs(monkeypatch, knobs)
    nv = _nv(dtype)
    n = (64 * 4 * 3 * cus * 2 + 64 * 5 + 3) * nv - 1       # more than 2 x (3 blocks per CU x 4 waves) chunks of 64 vectors
    p = 70
    what0 = f"pinned {np.dtype(dtype).name} {loss} {knobs}"
    X8, y, rng = _data(zlib.crc32(what0.encode()), n, p, dtype, list(range(p)))
    w = rng.integers(1, 4, size=n).astype(dtype) if loss == "wls" else None
    f = _make_loss(loss, dtype, X8, y, w)
    for B in (16, 32, 64):
        gl = gram_launch(n, dtype, B, cus, **_knob_args(knobs))
        if dtype == np.float32 and B == 64:
            assert gl["variant"] == "frag"
        elif B == 16 and knobs == "lt_short":
            assert gl["variant"] == "lt_long" and gl["CVN"] == 64
        else:
            assert gl["variant"] == knobs, gl
        assert gl["rounds"] >= 3 and gl["G"] == gl["Gmax"], gl
        m = p                                             # 64 + 6, 32 + 32 + 6, 4 x 16 + 6: full blocks after full blocks
        h, det = _run_pass(f"{what0} B={B} {gl['variant']}", f, X8, y, dtype, B, np.arange(1, m + 1), sqrt=loss == "sqrt")
        assert det.all() and _blocks(det, B) == [B] * (p // B) + [6], (what0, B, h)
        assert -(-B // (gl["PG"] * gl["CGN"])) >= 2 and 6 < gl["PG"] * gl["CGN"]     # whole rounds, then a partial one
    f.close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_default_policy_on_long_columns(monkeypatch, cus, dtype):
    """No knob set, at a column length the policy sends to the long-column variants: k_gramstep<T, NG, true> (64-vector
    chunks; fp64 B = 64 with its column pointers in LDS) from rounds64 >= kShortRounds, k_gramstep<T, 1, true> from 2e6
    rows, k_gramstep<T, 4> for fp32 B = 64.  One handle per storage type: the matrix is multi-gigabyte."""
    _set_knobs(monkeypatch, "default")
    nv = _nv(dtype)
    n = (64 * 16 * 4 * 2 * cus + 64 * 7 + 3) * nv - 1
    p = 70
    what0 = f"default long {np.dtype(dtype).name}"
    X8, y, _ = _data(zlib.crc32(what0.encode()), n, p, dtype, list(range(p)))
    f = _make_loss("ls", dtype, X8, y)
    want = {(np.float64, 64): ("lt_long", True), (np.float64, 32): ("lt_long", False), (np.float64, 16): ("lt_long", False),
            (np.float32, 64): ("frag", False), (np.float32, 32): ("lt_long", False), (np.float32, 16): ("lt_long", False)}
    for B in (64, 32, 16):
        gl = gram_launch(n, dtype, B, cus)
        assert n >= 2_000_000 and (gl["variant"], gl["ldscol"]) == want[(dtype, B)] and gl["CVN"] == 64, gl
        assert gl["rounds"] >= 16 and gl["G"] == gl["Gmax"], gl
        m = p
        h, det = _run_pass(f"{what0} B={B} {gl['variant']}", f, X8, y, dtype, B, np.arange(1, m + 1))
        assert det.all() and _blocks(det, B) == [B] * (p // B) + [6], (what0, B, h)
    f.close()


# ---- 3. / 4. how many coordinates move ------------------------------------------------------------------------------------
def _half_movers(rng, p, B, units):
    """About half of the coordinates, irregularly spread, such that no block's count is a multiple of any of `units`."""
    for _ in range(200):
        mask = rng.random(p) < 0.5
        mask[0] = True
        counts = [int(mask[i:i + B].sum()) for i in range(0, p, B)]
        if all(c >= 1 and all(c % u != 0 for u in units) for c in counts) and not mask[:B].all():
            return np.nonzero(mask)[0].tolist()
    raise AssertionError("no such pattern")


PATTERNS = ([(d, l, B, k) for d in DTYPES for B in (16, 32, 64) for l, k in (("ls", "default"), ("wls", "default"),
                                                                            ("ls", "frag"), ("ls", "lt_long"), ("ls", "lt_short"))
             if not (d == np.float32 and B == 64 and k in ("lt_long", "lt_short")) and not (B == 16 and k == "lt_short")]
            + [(np.float64, "sqrt", 64, "default"), (np.float32, "sqrt", 32, "default")])


@gpu
@pytest.mark.parametrize("dtype,loss,B,knobs", PATTERNS, ids=[f"{np.dtype(d).name}-{l}-{B}-{k}" for d, l, B, k in PATTERNS])
def test_wide_block_move_patterns(monkeypatch, cus, dtype, loss, B, knobs):
    """n = 4099 (the default policy takes the short-chunk variants <T, NG, true, 1> here, asserted).  All-move: nzp = B,
    more than one round of PG * CGN previous columns where the variant has them, nprev < B on the ragged last block
    (p = 70 for B = 64 and 32: the last block holds 6, and B = 32 runs a full block after a full one; p = 23 for B = 16).
    Half-move: h = 0 interleaved with h != 0, nzp not a multiple of PG or of
    8 (the clamp and the zeroed h of the last partial round, in k_gramstep and in k_multi_axpy).  One list that repeats a
    coordinate (the chunk_dup launch)."""
    _set_knobs(monkeypatch, knobs)
    n, p = 4099, 23 if B == 16 else 70
    last = p % B
    gl = gram_launch(n, dtype, B, cus, **_knob_args(knobs))
    if knobs == "default":
        want = "frag" if (B == 16 or (dtype == np.float32 and B == 64)) else "lt_short"
        assert gl["variant"] == want, gl
    else:
        assert gl["variant"] == knobs, gl
    what0 = f"pattern {np.dtype(dtype).name} {loss} B={B} {knobs}"
    X8, y, rng = _data(zlib.crc32(what0.encode()), n, p, dtype, list(range(p)), tie=(1, 3))
    w = rng.integers(1, 4, size=n).astype(dtype) if loss == "wls" else None
    f = _make_loss(loss, dtype, X8, y, w)
    visit = np.arange(1, p + 1)
    h, det = _run_pass(what0 + " all-move", f, X8, y, dtype, B, visit, sqrt=loss == "sqrt")
    assert det.all() and _blocks(det, B) == [B] * (p // B) + [last] and 0 < last < gl["PG"] * gl["CGN"], (what0, h)
    assert -(-B // (gl["PG"] * gl["CGN"])) >= 2, gl                       # more than one round of previous columns
    movers = _half_movers(rng, p, B, (gl["PG"], 8, gl["PG"] * gl["CGN"]))
    h, det = _run_pass(what0 + " half-move", f, X8, y, dtype, B, visit, movers=movers, sqrt=loss == "sqrt")
    nzp = _blocks(det, B)
    assert det.sum() == len(movers) and all(c >= 1 and c % gl["PG"] != 0 and c % 8 != 0 for c in nzp), (what0, nzp)
    assert nzp[0] % (gl["PG"] * gl["CGN"]) != 0 and not det[:B].all()
    if loss == "ls":
        dupv = visit.copy()
        dupv[B // 2 + 3] = 2                              # coordinate 2 again, later in the first block
        h, det = _run_pass(what0 + " repeated coordinate", f, X8, y, dtype, B, dupv)
        assert det[1] and det[B // 2 + 3] and all(c >= 1 for c in _blocks(det, B)), (what0, h)
    f.close()


NARROW = ([(d, l, "coord") for d in DTYPES for l in ("ls", "wls")] + [(np.float32, "sqrt", "coord")]
          + [(d, "ls", B) for d in DTYPES for B in (2, 4, 8)] + [(np.float64, "sqrt", 8)])


@gpu
@pytest.mark.parametrize("dtype,loss,mode", NARROW, ids=[f"{np.dtype(d).name}-{l}-{m}" for d, l, m in NARROW])
def test_narrow_block_and_coordinate_move_patterns(cus, dtype, loss, mode):
    """The per-coordinate sweep and B in {2, 4, 8} at n = 4099, p = 67 (m not a multiple of B): all-move, half-move (a
    launch after an unmoved visit must leave r alone), a repeated coordinate."""
    n, p = 4099, 67
    what0 = f"narrow {np.dtype(dtype).name} {loss} {mode}"
    assert mode == "coord" or p % mode != 0
    X8, y, rng = _data(zlib.crc32(what0.encode()), n, p, dtype, list(range(p)), tie=(1, 3))
    w = rng.integers(1, 4, size=n).astype(dtype) if loss == "wls" else None
    f = _make_loss(loss, dtype, X8, y, w)
    visit = np.arange(1, p + 1)
    h, det = _run_pass(what0 + " all-move", f, X8, y, dtype, mode, visit, sqrt=loss == "sqrt")
    assert det.all(), (what0, h)
    movers = np.nonzero(rng.random(p) < 0.5)[0].tolist()
    movers = sorted((set(movers) | {0, p - 1}) - {1, 3})       # (the tied pair stays: its moves can cancel each other)
    h, det = _run_pass(what0 + " half-move", f, X8, y, dtype, mode, visit, movers=movers, sqrt=loss == "sqrt")
    assert det.sum() == len(movers) and 2 < len(movers) < p, (what0, h)
    if loss == "ls":
        dupv = np.array([1, 2, 3, 4, 5, 6, 7, 8, 2, 9, 10, 11, 12])        # coordinate 2 again; 13 visits: ragged for every B
        h, det = _run_pass(what0 + " repeated coordinate", f, X8, y, dtype, mode, dupv)
        assert det[1] and det[8], (what0, h)
    f.close()


# ---- 5. sync_r's catch-up ---------------------------------------------------------------------------------------------------
def _served_by_the_cache_alone(f, st0, loop0):
    """The solve just finished ran every pass inside the device-resident loop, in covariance form: nothing was streamed (a
    streamed chunk would have applied the pending moves, or, with none pending yet, moved r without leaving any), and
    nothing has been applied to r yet."""
    st1, loop1 = f.cache_stats(), f.device_loop_stats()
    assert f.last_stats["passes"] >= 2, f.last_stats                                   # moves of a coordinate merge over passes
    assert loop1["passes"] - loop0["passes"] == f.last_stats["passes"], (loop0, loop1, f.last_stats)
    assert st1["covariance_visits"] > st0["covariance_visits"], (st0, st1)
    assert st1["residual_catchups"] == st0["residual_catchups"], (st0, st1)
    assert st1["rollbacks"] == st0["rollbacks"], (st0, st1)
    return st1


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("P", [100, 64, 65])
def test_catch_up_after_cache_served_solves(cus, dtype, P):
    """A warm-started solve served by the gradient cache moves P coordinates in covariance form and leaves them pending;
    reading f.r applies them with k_multi_axpy, 64 columns per launch: two batches with 36 = 4 * 8 + 4 in the second
    (P = 100), exactly one (64), one and a batch of a single column (65).  r was rebuilt by the solve's own initialize!
    (nnz + 1 operations, one store); the catch-up adds P moves and ceil(P / 64) stores.  Then once more after another
    solve on the same handle: what the first catch-up left in the pending ledger must be gone."""
    n, p = 6007, 4 * P + 40
    rng0 = np.random.default_rng(P)
    sup = np.sort(rng0.choice(p, size=P, replace=False)).tolist()
    X8, y, _ = _data(300 + P, n, p, dtype, sup)
    f = _make_loss("ls", dtype, X8, y)
    f.set_gradient_cache(3)
    x = cd.SparseIterate(p)
    o = cd.CDOptions(maxIter=300, optTol=1e-9 if dtype == np.float64 else 1e-6, randomize=False)
    cd.coordinateDescent_(x, f, cd.ProxL1(1.0), o)
    assert x.nnz == P and sorted((x.nzval2ind - 1).tolist()) == sup
    f.r                                                   # whatever is pending now is applied: the next solve starts clean
    for lam in (0.4, 0.15):
        b0, st0, loop0 = x.dense(), f.cache_stats(), f.device_loop_stats()
        cd.coordinateDescent_(x, f, cd.ProxL1(lam), o)
        st1 = _served_by_the_cache_alone(f, st0, loop0)
        r = f.r
        assert f.cache_stats()["residual_catchups"] == st1["residual_catchups"] + 1       # one reconcile
        b1 = x.dense()
        moved = b1 != b0
        assert int(moved.sum()) == P == x.nnz
        batches = -(-P // 64)
        bmax = _check(f"catch-up {np.dtype(dtype).name} P={P} lam={lam}", X8, y, dtype, r, b1, np.abs(b0) + np.abs(b1 - b0),
                      P + 1 + P, 1 + batches)
        det = np.abs(b1 - b0)[np.array(sup)] > DETECT * bmax
        assert det.all(), (P, lam, np.abs(b1 - b0)[np.array(sup)].min(), bmax)      # every batch holds detectable moves only
        assert int(det.sum()) == P and (P <= 64) == (batches == 1) and (P != 100 or (P - 64) % 8 != 0)
    f.close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("P", [100, 65])
def test_catch_up_of_moves_merged_over_several_solves(cus, dtype, P):
    """With the residual reused between warm starts (cdh_set_reuse_residual: what LassoPath runs by default) a solve does not
    rebuild r, so the moves of three cache-served solves in a row stay pending and merge, coordinate by coordinate, in
    the pending ledger; the list keeps the order the first of them gave it.  r is read once, at the end: it was last rebuilt by the
    first solve's initialize! (nnz + 1 operations, one store), and the catch-up applies one merged move per coordinate in
    ceil(P / 64) launches.  TV is summed solve by solve; the move applied is the net one, and every one of them -- so the
    second batch's too -- is detectable."""
    n, p = 6007, 4 * P + 40
    rng0 = np.random.default_rng(P + 1000)
    sup = np.sort(rng0.choice(p, size=P, replace=False)).tolist()
    X8, y, _ = _data(500 + P, n, p, dtype, sup)
    f = _make_loss("ls", dtype, X8, y)
    f.set_gradient_cache(3)
    x = cd.SparseIterate(p)
    o = cd.CDOptions(maxIter=300, optTol=1e-9 if dtype == np.float64 else 1e-6, randomize=False)
    cd.coordinateDescent_(x, f, cd.ProxL1(1.0), o)
    assert x.nnz == P and sorted((x.nzval2ind - 1).tolist()) == sup
    f.r
    b0 = x.dense()
    betas, st_first = [b0], f.cache_stats()
    for i, lam in enumerate((0.5, 0.3, 0.15)):
        if i == 1:
            check(f._L.cdh_set_reuse_residual(f._h, 1), f._h)       # from the second solve on: no initialize!, r is carried
        st0, loop0 = f.cache_stats(), f.device_loop_stats()
        cd.coordinateDescent_(x, f, cd.ProxL1(lam), o)
        _served_by_the_cache_alone(f, st0, loop0)
        betas.append(x.dense())
    st1 = f.cache_stats()
    assert st1["residual_catchups"] == st_first["residual_catchups"]        # three solves, nothing applied to r yet
    r = f.r
    assert f.cache_stats()["residual_catchups"] == st1["residual_catchups"] + 1
    check(f._L.cdh_set_reuse_residual(f._h, 0), f._h)
    steps = [np.abs(b - a) for a, b in zip(betas[:-1], betas[1:])]
    for d in steps:
        assert int((d != 0).sum()) == P                                      # every solve moved every coordinate: P merged entries
    merged = int((sum(steps) != 0).sum())
    batches = -(-merged // 64)
    assert merged == P == x.nnz and batches == 2
    bmax = _check(f"merged catch-up {np.dtype(dtype).name} P={P}", X8, y, dtype, r, betas[-1], np.abs(b0) + sum(steps),
                  P + 1 + merged, 1 + batches)
    net = np.abs(betas[-1] - b0)[np.array(sup)]
    assert np.all(net > DETECT * bmax), (P, net.min(), bmax)
    # had the three solves' moves been applied separately and not merged, the net move would still be right: what merging must
    # not do is lose one solve's share -- each share alone is detectable too
    for d in steps:
        assert np.all(d[np.array(sup)] > DETECT * bmax), (P, d[np.array(sup)].min(), bmax)
    f.close()
