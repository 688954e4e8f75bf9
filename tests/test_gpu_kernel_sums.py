"""The kernels that sum over rows, read directly: k_cross -> k_cross_reduce -> k_cross_unpack (the gradient cache's Gram
columns), k_gramstep run read-only with the pair stitching of cdh_gram, k_col_dots (cdh_xt_r, cdh_col_rms, cdh_xt_r_cols,
findLambdaMax) and k_resid_moments (cdh_resid_moments, cdh_resid_std, cdh_objective).

The main oracle is EXACTLY SUMMABLE data: small integers, so that every product and every partial sum any kernel can form
is representable.  The true result is then what numpy computes in fp64 in any order, and the kernel must match it bit for
bit whatever its own order -- a dropped or doubled sub-chunk, a row lane summed twice or a column written at the wrong
offset shows up as an integer-sized difference, not as rounding.  The fp32 kernels keep fp32 partial sums on the matrix
pipe, so their data range is derived below from the chain lengths in the code and asserted.  Each shape is chosen from
the device's CU count so that it reaches the indexing branch it is named for, and the test asserts that it does.  One
rounded-data case per kernel family checks the accuracy on real data against a bound written from the chain length.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
# the row chunks of the column dots and cdh_gram's grid: the twin of csrc/sweep_plan.hpp (tests/test_sweep_plan_host.py)
from _sweep_plan import col_dots_chunks, gram_grid  # noqa: F401  (test_gpu_generator takes them from here)

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53                      # unit roundoff of fp64
F64_XMAX, F64_YMAX, F64_WMAX = 2047, 2047, 3
# fp64 storage: every sum below has at most n terms of size xmax^2 wmax (or xmax ymax wmax); n <= 2^21 here
assert (1 << 21) * F64_XMAX * max(F64_XMAX, F64_YMAX) * F64_WMAX < 2 ** 53
# fp32 storage.  k_cross (gram_kernels.hpp) sums each Gram entry in an fp32 tile over kCrossFold * kX2SV * 4 = 8 * 8 * 4 =
# 256 rows before folding it into fp64 (the weight rides on the B operand: x_j w in fp32).  k_gramstep (cdh_gram) folds its
# fp32 Gram tiles every 64-vector chunk = 256 rows, and its per-lane X_I'r partial c32 (fmaf, B >= 32) takes the lane's 16
# vectors of the chunk = 64 rows.  k_col_dots and k_resid_moments accumulate in fp64 from the start.  So |x| <= 127,
# w <= 3 and |y| <= 511 keep every fp32 partial sum an integer below 2^24:
F32_XMAX, F32_YMAX, F32_WMAX = 127, 511, 3
CROSS_F32_CHAIN, GRAMSTEP_F32_CHAIN, GRAMSTEP_C32_CHAIN = 256, 256, 64
assert CROSS_F32_CHAIN * F32_XMAX * F32_XMAX * F32_WMAX < 2 ** 24
assert GRAMSTEP_F32_CHAIN * F32_XMAX * F32_XMAX < 2 ** 24
assert GRAMSTEP_C32_CHAIN * F32_XMAX * F32_YMAX < 2 ** 24


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nv(dtype):
    return 2 if dtype == np.float64 else 4          # elements per 16-byte vector


def _ints(rng, n, p, dtype):
    """n x p Fortran-order integer-valued X (no zero entries, so that no column of a short X is all zero)."""
    xmax = F64_XMAX if dtype == np.float64 else F32_XMAX
    raw = rng.integers(-xmax, xmax + 1, size=(p, n), dtype=np.int16 if dtype == np.float64 else np.int8)
    raw[raw == 0] = 1
    return raw.T.astype(dtype)                        # (p, n) C-order transposed: Fortran order, kept by astype


def _int_y(rng, n, dtype):
    ymax = F64_YMAX if dtype == np.float64 else F32_YMAX
    return rng.integers(-ymax, ymax + 1, size=n).astype(dtype)


def _weights(rng, n, dtype):
    return rng.integers(0, F64_WMAX + 1, size=n).astype(dtype)


def _loss(kind, y, X, w=None):
    if kind == "wls":
        return cd.CDWeightedLSLoss(y, X, w)
    return {"ls": cd.CDLeastSquaresLoss, "sqrt": cd.CDSqrtLassoLoss}[kind](y, X)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- grids, restated from the host code ----------------------------------------------------------------------------
def cross_grid(n, p, dtype, cus):
    """k_cross's launch as grad_cache.hpp:gc_size sizes it, and the branches gram_kernels.hpp:k_cross takes on it."""
    nvec = -(-n // _nv(dtype))
    nslabs = -(-nvec // 1024)                          # kCrossSlab vectors per row slab
    ngroups = -(-p // 64)                              # kCrossA columns per group
    nsuper = -(-ngroups // 4)                          # kGramWaves groups per super-group
    occ = 2 if dtype == np.float32 else 3              # cross_occ<T>()
    gx = max(1, min(nsuper, 4))
    J = max(1, min(nslabs, occ * cus // gx))
    gx = min(nsuper, max(gx, occ * cus // J))
    return {"nvec": nvec, "nslabs": nslabs, "nsuper": nsuper, "GX": gx, "J": J,
            "remap": J % 8 == 0,                        # the XCD remap of (blockIdx.x, blockIdx.y)
            "lanes_walk_slabs": nslabs > J,             # a row lane sums several slabs
            "blocks_walk_supergroups": nsuper > gx,     # the sg += gridDim.x loop
            "partial_last_slab": nvec % 1024 != 0,
            "partial_last_subchunk": nvec % 8 != 0,     # kX2SV vectors per sub-chunk
            "rows_per_lane": -(-nslabs // J) * 1024 * _nv(dtype)}


# ---- 2. Gram columns: k_cross -> k_cross_reduce -> k_cross_unpack via the gradient cache -----------------------------
# (p = 1 is not here: the cache serves full passes of at least kScreenMinPass = 16 coordinates)
def _shape(case, dtype, cus):
    R = 1024 * _nv(dtype)                              # rows per row slab
    occ = 2 if dtype == np.float32 else 3
    # blocks walking super-groups with the remap on: J = occ cus / 4 row lanes once there are that many slabs (one slab
    # more: the lanes walk slabs too) -- or, where that J is not a multiple of 8, the largest multiple of 8 below it --
    # and one super-group more than the GX = max(4, occ cus / J) the grid has
    cap = occ * cus // 4
    walk_n = cap * R + 1000 if cap % 8 == 0 else (cap // 8 * 8) * R - 1000
    walk_p = 256 * max(4, occ * cus // (cap if cap % 8 == 0 else cap // 8 * 8)) + 1
    return {
        "p63_clamped_columns": (3000, 63), "p64_one_group": (3000, 64), "p65_clamped_columns": (3000, 65),
        "p257_lone_supergroup_column": (3000, 257),
        "n1": (1, 65), "n15": (15, 65), "n2047": (2047, 65), "n2048": (2048, 65), "n2049": (2049, 65),
        "n4095": (4095, 65), "n4096": (4096, 65), "n4097": (4097, 65),
        "remap": ((8 * 1024 - 3) * _nv(dtype) - 1, 65),             # 8 row slabs, the last one partial
        "lanes_walk_slabs": (occ * cus * R + 5, 24),
        "blocks_walk_supergroups": (walk_n, walk_p),     # 256 CUs: fp64 394 216 x 1025, fp32 525 288 x 1025
    }[case]


def occ_cus(dtype, cus):
    return (2 if dtype == np.float32 else 3) * cus


def _branch_holds(case, g, n, p, dtype, cus):
    """Each shape reaches the branch it is named for (a later retune of the grid must not turn it into a duplicate)."""
    nv = _nv(dtype)
    want = {
        "p63_clamped_columns": p % 64 != 0,
        "p64_one_group": p == 64 and g["nsuper"] == 1,
        "p65_clamped_columns": p % 64 == 1 and g["nsuper"] == 1,
        "p257_lone_supergroup_column": p % 256 == 1 and g["nsuper"] == 2,
        "n1": g["nvec"] == 1 and g["partial_last_subchunk"],
        "n15": n % nv != 0 and g["nvec"] % 8 == 0 and g["nslabs"] == 1,        # pad row inside a whole sub-chunk
        "n2047": g["nvec"] == 1024 and n % nv != 0,                            # one whole slab, its last vector padded
        "n2048": g["nvec"] == 1024 and n % nv == 0,
        "n2049": g["nslabs"] == 2 and g["partial_last_subchunk"],
        "n4095": g["nvec"] == 1024 and n % nv != 0,
        "n4096": g["nvec"] == 1024 and n % nv == 0,
        "n4097": g["nslabs"] == 2 and g["partial_last_subchunk"],
        "remap": g["remap"] and g["J"] == 8 and not g["lanes_walk_slabs"] and g["partial_last_slab"],
        "lanes_walk_slabs": g["lanes_walk_slabs"] and g["partial_last_slab"],
        "blocks_walk_supergroups": g["blocks_walk_supergroups"] and g["remap"] and g["partial_last_slab"]
                                   and (g["lanes_walk_slabs"] or (occ_cus(dtype, cus) // 4) % 8 != 0),
    }[case]
    assert want, (case, n, p, g)


def _xt_dot(X, B, w=None, rows=1 << 16):
    """X'WB and diag(X'WX) in fp64, over blocks of rows (no fp64 copy of a large fp32 X).  Integer data: exact."""
    out, a = np.zeros((X.shape[1], B.shape[1])), np.zeros(X.shape[1])
    for i0 in range(0, X.shape[0], rows):
        Xb = X[i0:i0 + rows].astype(np.float64, copy=False)
        Wb = Xb if w is None else Xb * w[i0:i0 + rows].astype(np.float64)[:, None]
        out += Wb.T @ B[i0:i0 + rows].astype(np.float64, copy=False)
        a += np.einsum("ij,ij->j", Wb, Xb)
    return out, a


def _cached_gram_columns(f, p):
    cols = {}
    for k in range(1, p + 1):
        try:
            cols[k] = f.cache_gram_column(k)
        except cd.ArgumentError:
            pass
    return cols


def _planted_solve(f, X, y, w=None):
    """Solve with the gradient cache forced: the planted coordinates move, and the cache fetches their Gram columns."""
    n, p = X.shape
    f.set_gradient_cache(3)
    f.set_onchip_solve(False)
    wy = y if w is None else y * w
    lam = 0.3 * float(np.max(np.abs(X.T @ wy))) / n                  # the planted coordinates enter, the others mostly not
    x = cd.SparseIterate(p)
    cd.coordinateDescent_(x, f, cd.ProxL1(lam), cd.CDOptions(maxIter=100, optTol=1e-7, randomize=False))
    return x


def _planted_y(X, rng, s, dtype):
    n = X.shape[0]
    beta = (1.0 + rng.random(s)) * rng.choice([-1.0, 1.0], size=s)
    y = X[:, :s].astype(np.float64) @ beta + 0.3 * float(np.abs(X[:, 0]).max()) * rng.standard_normal(n)
    return y.astype(dtype)


GRAM_CASES = (
    [(np.float64, "ls", c) for c in ("p63_clamped_columns", "p64_one_group", "p65_clamped_columns",
                                      "p257_lone_supergroup_column", "n1", "n15", "n2047", "n2048", "n2049", "remap",
                                      "lanes_walk_slabs", "blocks_walk_supergroups")]
    + [(np.float64, "wls", c) for c in ("p65_clamped_columns", "p257_lone_supergroup_column", "n15", "n2049", "remap")]
    + [(np.float32, "ls", c) for c in ("p63_clamped_columns", "p257_lone_supergroup_column", "n4095", "n4096", "n4097",
                                        "remap")]
    + [(np.float32, "wls", c) for c in ("p65_clamped_columns", "n4097", "remap", "lanes_walk_slabs")]
)


@pytest.mark.parametrize("dtype,loss,case", GRAM_CASES,
                         ids=[f"{np.dtype(d).name}-{l}-{c}" for d, l, c in GRAM_CASES])
def test_gram_columns_are_exact_on_integer_data(cus, dtype, loss, case):
    """Every Gram column the gradient cache holds, over all p entries, equals X'X_k (X'WX_k) summed exactly on the host."""
    n, p = _shape(case, dtype, cus)
    g = cross_grid(n, p, dtype, cus)
    _branch_holds(case, g, n, p, dtype, cus)
    rng = np.random.default_rng(zlib.crc32(f"{np.dtype(dtype).name}-{loss}-{case}".encode()))
    X = _ints(rng, n, p, dtype)
    s = min(40, p // 6)                 # (a full pass is screened, and so served by the cache, while nnz <= p / 4)
    y = _planted_y(X, rng, s, dtype)
    w = _weights(rng, n, dtype) if loss == "wls" else None
    f = _loss(loss, y, X, w)
    x = _planted_solve(f, X, y, w)
    cached = _cached_gram_columns(f, p)
    st = f.cache_stats()
    assert len(cached) == st["gram_columns"] > 0, st
    assert set(x.nzval2ind.tolist()) <= set(cached), (x.nzval2ind.tolist(), sorted(cached))
    if s > 32:
        assert st["gram_batches"] >= 2 and len(cached) > 32, st       # a full batch of 32 and a partial one
    ks = np.array(sorted(cached)) - 1
    exact, a = _xt_dot(X, X[:, ks], w)                                  # integer sums < 2^53: exact in any order
    got = np.stack([cached[k + 1][0] for k in ks], axis=1)
    np.testing.assert_array_equal(got, exact)
    np.testing.assert_array_equal(got[ks, np.arange(len(ks))], a[ks])   # G_kk = a_k
    f.close()


def test_fp64_gram_columns_on_rounded_data_stay_within_the_chain_bound(cus):
    """standard_normal data at a remapped grid: |G - X'X_k| <= 4 L 2^-53 sqrt(a_i a_k), L the longest sequential chain of
    k_cross (the rows of one row lane, one MFMA step per 4 of them, plus the J records k_cross_reduce adds), against a
    long-double reference."""
    dtype = np.float64
    n, p = _shape("remap", dtype, cus)
    p = 257
    g = cross_grid(n, p, dtype, cus)
    assert g["remap"] and g["nsuper"] == 2
    L = g["rows_per_lane"] + g["J"] + 2
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = X[:, :12] @ rng.standard_normal(12) + rng.standard_normal(n)
    f = cd.CDLeastSquaresLoss(y, X)
    f.set_gradient_cache(3)
    f.set_onchip_solve(False)
    x = cd.SparseIterate(p)
    cd.coordinateDescent_(x, f, cd.ProxL1(0.05), cd.CDOptions(maxIter=100, optTol=1e-8, randomize=False))
    cached = _cached_gram_columns(f, p)
    assert len(cached) == f.cache_stats()["gram_columns"] >= x.nnz > 0
    ks = np.array(sorted(cached)) - 1
    XL = X.astype(np.longdouble)
    exact = XL.T @ XL[:, ks]
    a = np.einsum("ij,ij->j", X, X)
    for j, k in enumerate(ks):
        col, eps = cached[k + 1]
        assert eps == 0.0
        err = np.max(np.abs(col - exact[:, j]).astype(np.float64) / np.sqrt(a * a[k]))
        assert err <= 4 * L * U64, (k, err, L)
    f.close()


def test_fp32_gram_columns_at_the_walking_shape_carry_the_declared_error(cus):
    """fp32 storage on standard_normal data where blocks walk several super-groups and the remap is on: every cached entry
    stays under the error cdh_cache_gram_column declares (2^-24 * 512 / sqrt(n), in units of sqrt(a_i a_k))."""
    dtype = np.float32
    n, p = _shape("blocks_walk_supergroups", dtype, cus)
    g = cross_grid(n, p, dtype, cus)
    _branch_holds("blocks_walk_supergroups", g, n, p, dtype, cus)
    rng = np.random.default_rng(6)
    X = np.asfortranarray(rng.standard_normal((p, n), dtype=np.float32).T)
    X[:, 5] = X[:, 4] * np.float32(1.5)                 # fully correlated: the worst case of the bound
    y = _planted_y(X, rng, 40, dtype)
    f = cd.CDLeastSquaresLoss(y, X)
    x = _planted_solve(f, X, y)
    cached = _cached_gram_columns(f, p)
    assert len(cached) == f.cache_stats()["gram_columns"] >= 32 and x.nnz > 0      # at least one whole batch
    ks = np.array(sorted(cached)) - 1
    exact, a = _xt_dot(X, X[:, ks])          # fp32 products are exact in fp64; the fp64 sums err by ~n 2^-53 << eps
    for j, k in enumerate(ks):
        col, eps = cached[k + 1]
        assert eps == pytest.approx(2.0 ** -24 * 512 / np.sqrt(n))
        err = np.max(np.abs(col - exact[:, j]) / np.sqrt(a * a[k]))
        assert err <= eps, (k, err, eps)
    f.close()


# ---- 3. cdh_gram: k_gramstep read-only, one launch (m <= 64) or pairs of 32-column groups ---------------------------
GRAM_MS = (1, 16, 17, 63, 64, 65, 95, 96, 97, 128, 129)


def _cdh_gram(f, idx1):
    m = len(idx1)
    idx1 = np.ascontiguousarray(idx1, dtype=np.int64)
    G, c, q = np.zeros((m, m)), np.zeros(m), C.c_double()
    cd._lib.check(f._L.cdh_gram(f._h, m, _vp(idx1), _vp(G), _vp(c), C.byref(q)), f._h)
    return G, c, q.value


def _index_list(rng, m, p):
    """m distinct columns, unsorted, holding column 1 and column p whenever m >= 2."""
    if m == 1:
        return np.array([p])
    rest = rng.choice(np.arange(2, p), size=m - 2, replace=False)
    idx = np.concatenate([[1, p], rest])
    rng.shuffle(idx)
    return idx


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("n", [1, 31, 33, 5003, 1_000_003])
def test_gram_entry_point_is_exact_on_integer_data(cus, dtype, n):
    p = 130
    G_blocks, nchunks = gram_grid(n, dtype, cus)
    if n == 1_000_003:
        assert nchunks > 4 * G_blocks                   # every wave of every block walks more than one chunk
    rng = np.random.default_rng(n + (0 if dtype == np.float64 else 7))
    X = _ints(rng, n, p, dtype)
    y = _int_y(rng, n, dtype)
    f = cd.CDLeastSquaresLoss(y, X)
    y64 = y.astype(np.float64)
    Gall, _ = _xt_dot(X, X)                                             # exact: integer sums < 2^53
    call, _ = _xt_dot(X, y64[:, None])
    call, qall = call[:, 0], float(y64 @ y64)
    for m in GRAM_MS:
        idx = _index_list(rng, m, p)
        G, c, q = _cdh_gram(f, idx)
        np.testing.assert_array_equal(G, Gall[np.ix_(idx - 1, idx - 1)], err_msg=f"m={m}")
        np.testing.assert_array_equal(G, G.T, err_msg=f"m={m}")
        np.testing.assert_array_equal(c, call[idx - 1], err_msg=f"m={m}")
        assert q == qall, m
    np.testing.assert_array_equal(f.r, y)               # r is only read
    f.close()


def test_gram_and_xt_r_catch_up_with_the_moves_a_cache_served_solve_leaves_pending():
    """After a solve served by the gradient cache the residual has moves pending (sync_r).  cdh_gram's c and cdh_xt_r must
    describe y - X beta for the beta the solve returned.  beta is no longer integer, so the host's X'(y - X beta) is compared
    within the rounding of the device's residual: each of the at most W updates of r rounds an element by 2^-53 of
    |y_i| + sum_j |x_ij beta_j|, and the dot adds a chain of n; a move left out is of the size of the moves themselves."""
    n, p = 5003, 140
    rng = np.random.default_rng(11)
    X = _ints(rng, n, p, np.float64)
    y = _planted_y(X, rng, 20, np.float64)
    f = cd.CDLeastSquaresLoss(y, X)
    f.set_gradient_cache(3)
    f.set_onchip_solve(False)
    x = cd.SparseIterate(p)
    lam_max = float(np.max(np.abs(X.T @ y))) / n
    o = cd.CDOptions(maxIter=200, optTol=1e-9, randomize=False)

    def host_r(beta):
        return y - X @ beta

    def tol(beta):
        W = (f.last_stats["passes"] + 2) * p
        scale = np.abs(X).T @ (np.abs(y) + np.abs(X) @ np.abs(beta))
        return (W + n) * U64 * scale

    cd.coordinateDescent_(x, f, cd.ProxL1(0.2 * lam_max), o)
    st0 = f.cache_stats()
    assert x.nnz > 0 and st0["passes"] > 0, st0
    idx = _index_list(rng, 97, p)                       # the pair path
    G, c, q = _cdh_gram(f, idx)
    assert f.cache_stats()["residual_catchups"] > st0["residual_catchups"]
    beta = x.dense()
    r = host_r(beta)
    np.testing.assert_array_equal(G, (X.T @ X)[np.ix_(idx - 1, idx - 1)])
    assert np.all(np.abs(c - X[:, idx - 1].T @ r) <= tol(beta)[idx - 1])
    cd.coordinateDescent_(x, f, cd.ProxL1(0.05 * lam_max), o)          # more moves pending, then X'r over all p
    st1 = f.cache_stats()
    out = np.zeros(p)
    cd._lib.check(f._L.cdh_xt_r(f._h, _vp(out)), f._h)
    assert f.cache_stats()["residual_catchups"] > st1["residual_catchups"], (st1, f.cache_stats())
    beta = x.dense()
    assert np.all(np.abs(out - X.T @ host_r(beta)) <= tol(beta))
    f.close()


def test_gram_entry_point_on_rounded_data_stays_within_the_chain_bound(cus):
    """standard_normal fp64 data, both paths: |G - X_S'X_S| <= 4 L 2^-53 sqrt(a_i a_j) and |c - X_S'y| <= 4 L 2^-53 |x_i| |y|,
    L the longest chain of k_gramstep (the rows of the chunks one wave takes, the 4 waves, the G block records summed)."""
    n, p = 100_003, 130
    G_blocks, nchunks = gram_grid(n, np.float64, cus)
    L = -(-nchunks // (4 * G_blocks)) * 128 + 4 + G_blocks
    rng = np.random.default_rng(12)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = rng.standard_normal(n)
    f = cd.CDLeastSquaresLoss(y, X)
    a, yyL = np.einsum("ij,ij->j", X, X), y.astype(np.longdouble) @ y.astype(np.longdouble)
    yy = float(yyL)
    for m in (64, 129):
        idx = _index_list(rng, m, p) - 1
        XL = X[:, idx].astype(np.longdouble)
        G, c, q = _cdh_gram(f, idx + 1)
        errG = np.abs(G - XL.T @ XL).astype(np.float64) / np.sqrt(np.outer(a[idx], a[idx]))
        errc = np.abs(c - XL.T @ y.astype(np.longdouble)).astype(np.float64) / np.sqrt(a[idx] * yy)
        assert errG.max() <= 4 * L * U64 and errc.max() <= 4 * L * U64, (m, errG.max(), errc.max(), L)
        assert abs(float(q - yyL)) <= 4 * L * U64 * yy
    f.close()


# ---- 4. column dots and residual moments ---------------------------------------------------------------------------
def _colchunk_case(case, dtype):
    """(n, p, the chunk counts the launches must reach); None: whatever the formula gives (the case is about batches)."""
    return {
        "p4095": (37, 4095, None), "p4096": (37, 4096, None), "p4097": (37, 4097, None), "p8193": (37, 8193, None),
        "n1": (1, 20, [1]), "n3": (3, 20, [1]),
        "n512_one_stride": (256 * _nv(dtype), 20, [1]),
        "n_second_stride_mid_vector": (256 * _nv(dtype) + 1, 20, [2]),
        "n_mid_stride": (1000 * _nv(dtype) - 1, 20, [4]),
        "n_64_chunks_mid_stride": (64 * 256 * _nv(dtype) * 3 + 517, 20, [64]),
    }[case]


COLDOT_CASES = ([(np.float64, c) for c in ("p4095", "p4096", "p4097", "p8193", "n1", "n3", "n512_one_stride",
                                            "n_second_stride_mid_vector", "n_mid_stride", "n_64_chunks_mid_stride")]
                + [(np.float32, c) for c in ("p4097", "p8193", "n1", "n_second_stride_mid_vector", "n_mid_stride")]
                + [(np.float32, "n4M")])


@pytest.mark.parametrize("dtype,case", COLDOT_CASES, ids=[f"{np.dtype(d).name}-{c}" for d, c in COLDOT_CASES])
def test_column_dots_are_exact_on_integer_data(cus, dtype, case):
    """cdh_xt_r (X'r), cdh_col_rms (sqrt(a_k / n)) and findLambdaMax (max |X_k'r| / n), r = y, against exact sums."""
    if case == "n4M":
        n, p, want = 4_000_003, 20, [64]
    else:
        n, p, want = _colchunk_case(case, dtype)
    chunks = col_dots_chunks(n, p, dtype, cus)
    if want is not None:
        assert chunks == want, (case, chunks)
    if p > 4096:
        assert len(chunks) == -(-p // 4096) and p % 4096 != 0   # batches written at an offset, the last one short
    rng = np.random.default_rng(p * 7 + n)
    X = _ints(rng, n, p, dtype)
    y = _int_y(rng, n, dtype)
    f = cd.CDLeastSquaresLoss(y, X)
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    xty, a = X64.T @ y64, np.einsum("ij,ij->j", X64, X64)
    out = np.zeros(p)
    cd._lib.check(f._L.cdh_xt_r(f._h, _vp(out)), f._h)
    np.testing.assert_array_equal(out, xty)
    np.testing.assert_array_equal(cd.stdX(f), np.sqrt(a / float(n)))
    lmax = cd.findLambdaMax(cd.SparseIterate(p), f, cd.ProxL1(1.0))
    assert lmax == float(np.max(np.abs(-xty / float(n))))
    f.close()


def test_column_dots_on_rounded_data_stay_within_the_chain_bound(cus):
    """standard_normal fp64: |X_k'r - exact| <= 4 L 2^-53 |x_k| |r|, L = the rows one thread sums, the block's tree, the
    chunks k_col_dots_reduce adds."""
    n, p = 100_003, 20
    (chunks,) = col_dots_chunks(n, p, np.float64, cus)
    nvec = -(-n // 2)
    L = -(-nvec // (chunks * 256)) * 2 + 8 + chunks
    rng = np.random.default_rng(13)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = rng.standard_normal(n)
    f = cd.CDLeastSquaresLoss(y, X)
    out = np.zeros(p)
    cd._lib.check(f._L.cdh_xt_r(f._h, _vp(out)), f._h)
    exact = (X.astype(np.longdouble).T @ y.astype(np.longdouble))
    err = np.abs(out - exact).astype(np.float64) / np.sqrt(np.einsum("ij,ij->j", X, X) * float(y @ y))
    assert err.max() <= 4 * L * U64, (err.max(), L)
    f.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_weighted_xt_r_cols_over_more_columns_than_p_with_duplicates(dtype):
    """cdh_xt_r_cols on CDWeightedLSLoss is X_S'Wr, chunked by p when the list is longer than p (m = 100 > p = 40)."""
    n, p, m = 3001, 40, 100
    rng = np.random.default_rng(14)
    X, y, w = _ints(rng, n, p, dtype), _int_y(rng, n, dtype), _weights(rng, n, dtype)
    f = cd.CDWeightedLSLoss(y, X, w)
    idx1 = rng.integers(1, p + 1, size=m).astype(np.int64)
    idx1[[3, 50, 99]] = idx1[7]                          # duplicates, across the p-sized chunks
    out = np.zeros(m)
    cd._lib.check(f._L.cdh_xt_r_cols(f._h, m, _vp(idx1), _vp(out)), f._h)
    exact = X.astype(np.float64).T @ (w.astype(np.float64) * y.astype(np.float64))
    np.testing.assert_array_equal(out, exact[idx1 - 1])
    f.close()


@pytest.mark.parametrize("loss", ["ls", "sqrt", "wls"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("n", [1, 7, 1025, 600_001])
def test_residual_moments_std_and_objective_are_exact_on_integer_data(loss, dtype, n):
    """k_resid_moments at beta = 0 (r = y): cdh_resid_moments against the exact sums; cdh_resid_std and cdh_objective
    against the host formulas applied to them.  y's mean is made an exact integer, so that the shifted second pass of
    cdh_resid_std (which must leave the zero pad rows out) sums exact values too."""
    rng = np.random.default_rng(n * 3 + len(loss))
    y = _int_y(rng, n, dtype).astype(np.float64)
    y[-1] -= y.sum() - 3 * n                             # sum(y) = 3 n: the mean is exactly 3 (|y[-1]| stays below 2^24)
    y = y.astype(dtype)
    assert float(y.astype(np.float64).sum()) == 3.0 * n
    X = _ints(rng, n, 3, dtype)
    w = _weights(rng, n, dtype)
    f = _loss(loss, y, X, w)
    y64, w64 = y.astype(np.float64), w.astype(np.float64)
    s, ss = C.c_double(), C.c_double()
    cd._lib.check(f._L.cdh_resid_moments(f._h, C.byref(s), C.byref(ss)), f._h)
    assert (s.value, ss.value) == (float(y64.sum()), float(y64 @ y64))
    if n > 1:
        sd, mean = C.c_double(), C.c_double()
        cd._lib.check(f._L.cdh_resid_std(f._h, C.byref(sd), C.byref(mean)), f._h)
        yc = y64 - 3.0
        assert mean.value == 3.0
        assert sd.value == np.sqrt(max(float(yc @ yc) - 0.0 * 0.0 / n, 0.0) / (n - 1.0))
    obj = cd.objective(f, cd.ProxL1(0.5))
    want = {"ls": float(y64 @ y64) / (2.0 * n), "sqrt": float(np.sqrt(y64 @ y64)),
            "wls": float(y64 @ (w64 * y64)) / (2.0 * n)}[loss]
    assert obj == want, (obj, want)
    f.close()
