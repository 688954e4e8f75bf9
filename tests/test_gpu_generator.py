"""cdh_generate read directly: k_gen_X, k_gen_y and struct Philox (csrc/kernels.hpp) and the host loop that plants beta*
(cdhip.hip), entry by entry against the numpy twin of tests/_philox_numpy.py.

The twin reproduces Philox and the uniforms bit for bit; Box-Muller goes through the device's log, sqrt and sincos, so an
fp64 entry is held to |X_dev - x_longdouble| <= ULPS 2^-53 rad (ULPS = 8: a ceiling for a library that meets 1 ulp for log
and 2 ulp for sincos, about 3.5 in all) and an fp32 entry to bit equality with np.float32(x_longdouble), the neighbouring
float admitted only where the longdouble value lies that close to an fp32 rounding boundary.  A keying or indexing mistake
is another normal altogether: off by the order of 1, about 1e15 of these units (tests/test_philox_host.py puts six such
mistakes into the twin and shows that this comparison catches each).

Shapes are the smallest that reach each branch: 512 rows are the 256 row pairs of one block of k_gen_X; n > 2^20 makes
both kernels' grid-stride loops wrap; p > 32 768 reaches the second column slice; a shard at global row 2^33 makes the
high word of the counter non-zero (only the n_local rows of a shard are allocated).  Each case prints its figures
(`GENFIG ...`) before it asserts.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (for the CU count; torch finds no GPU if it is first imported after the library has loaded HIP)

import coordinatedescent_jl_amd as cd

import _philox_numpy as P

pytestmark = pytest.mark.gpu

SEEDS = (123, 7)
DTYPES = (np.float64, np.float32)
L = np.longdouble
CDH_BAD_ARG = 2


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _ids(cases):
    return ["-".join(np.dtype(c).name if isinstance(c, type) else str(c) for c in case) for case in cases]


def _generate(n, p, seed, s, noise, dtype, cls=None, **kw):
    return (cls or cd.CDLeastSquaresLoss).generate(n, p, seed=seed, s=s, noise=noise, dtype=dtype, **kw)


def _regenerate(f, seed, s, noise):
    """cdh_generate on a handle that exists: -> (status, beta*)."""
    bstar = np.zeros(max(int(s), 1))
    status = f._L.cdh_generate(f._h, int(seed), int(s), float(noise), _vp(bstar))
    f._synced = None
    return status, bstar[: max(int(s), 0)]


@functools.lru_cache(maxsize=2)
def _x_ref(seed, row0, n, col0, p):
    """(longdouble reference, rad) of a block of X; computed once for the fp64 and the fp32 case that share it."""
    _, ref, rad = P.x_matrix(seed, row0, n, col0, p)
    ref.setflags(write=False)
    rad.setflags(write=False)
    return ref, rad


@functools.lru_cache(maxsize=2)
def _noise_ref(seed, row0, n):
    _, ref, rad = P.noise_vector(seed, row0, n)
    ref.setflags(write=False)
    rad.setflags(write=False)
    return ref, rad


def _fig(case, **kw):
    print("GENFIG " + case + " " + " ".join(f"{k}={v}" for k, v in kw.items()), flush=True)


def _differ(a, b):
    """Two draws that share nothing: independent normals coincide in an entry only by accident of rounding (about 1e-8 of
    fp32 entries), so all but a hundredth of the entries differ -- a repeated block would be equal throughout."""
    return a.shape == b.shape and float(np.mean(a == b)) < 0.01


def _check_X(case, X, seed, row0, col0=0, name_rows=(), name_cols=()):
    """Every entry of a downloaded block against the twin; the named rows / columns are spelled out on failure."""
    n, p = X.shape
    ref, rad = _x_ref(seed, row0, n, col0, p)
    bad, fig = P.check_x(X, ref, rad)
    _fig(case, what="X", dtype=X.dtype.name, seed=seed, n=n, p=p, **fig)
    if bad.any():
        rows, cols = np.nonzero(bad)
        msg = [f"{case}: {bad.sum()} of {bad.size} entries of X differ from the twin; first at local row {rows[0]} "
               f"(global {row0 + rows[0]}), column {col0 + cols[0]}: device {X[rows[0], cols[0]]!r}, "
               f"reference {float(ref[rows[0], cols[0]])!r}"]
        msg += [f"row {i}: {'WRONG' if bad[i].any() else 'ok'}" for i in name_rows]
        msg += [f"column {col0 + j}: {'WRONG' if bad[:, j].any() else 'ok'}" for j in name_cols]
        pytest.fail("; ".join(msg))
    return fig


def _check_beta_star(bstar, seed, s):
    """beta* is planted on the host, with the host's separate sin and cos: the same ceiling, relative to |z| (1 + u1)."""
    assert bstar.shape == (s,)
    _, ref, scale = P.beta_star(seed, s)
    err = np.abs(bstar.astype(L) - ref).astype(np.float64)
    assert np.all(err <= P.ULPS * P.U64 * scale), (bstar, ref)


def _check_y(case, f, X, bstar, seed, row0, noise, exact_chain=True, name_rows=()):
    """y against the fma chain over the DOWNLOADED (stored) X and the returned beta*, plus noise times the twin's e; r is a
    bitwise copy of y.  exact_chain: the chain is replayed exactly (small n); otherwise a longdouble dot stands in for it,
    and the chain's own rounding, s 2^-53 sum |x_j b_j| (tests/test_philox_host.py), is added to what is allowed."""
    y, r = f.y, f.r
    n, s = X.shape[0], len(bstar)
    assert y.dtype == X.dtype and r.dtype == X.dtype
    np.testing.assert_array_equal(r.view(np.uint8), y.view(np.uint8), err_msg=f"{case}: r is not a bitwise copy of y")
    assert np.all(np.isfinite(y))
    Xs = X[:, :s]
    if exact_chain:
        acc, slack = P.y_exact(Xs, bstar), 0.0
    else:
        acc = (Xs.astype(L) * bstar.astype(L)).sum(axis=1)
        slack = s * P.U64 * (np.abs(Xs.astype(np.float64)) * np.abs(bstar)).sum(axis=1)
    if noise == 0.0:
        assert exact_chain
        np.testing.assert_array_equal(y, acc.astype(y.dtype), err_msg=f"{case}: y is not the fma chain over the stored X")
        return
    eL, erad = _noise_ref(seed, row0, n)
    err = np.abs(y.astype(L) - (acc.astype(L) + L(noise) * eL)).astype(np.float64)
    spacing = np.spacing(np.abs(y)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        units = np.where(err <= spacing + slack, 0.0, (err - spacing - slack) / (P.U64 * abs(noise) * erad))
    _fig(case, what="y", dtype=y.dtype.name, seed=seed, n=n, s=s, **{"max_err_in_2^-53_noise_rad": float(units.max())})
    bad = ~(units <= P.ULPS)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        msg = [f"{case}: {bad.sum()} of {n} entries of y are off; first at local row {i}: device {y[i]!r}, "
               f"chain + noise {float(acc[i] + noise * eL[i])!r}"]
        msg += [f"row {i}: {'WRONG' if bad[i] else 'ok'}" for i in name_rows]
        pytest.fail("; ".join(msg))


# ---- 1. small shapes, every entry ------------------------------------------------------------------------------------
SMALL = [(n, seed, dt) for n in (1, 2, 3, 31, 32, 33, 511, 512, 513) for seed in SEEDS for dt in DTYPES]


@pytest.mark.parametrize("n,seed,dtype", SMALL, ids=_ids(SMALL))
def test_small_shapes_every_entry(n, seed, dtype):
    p, s = 5, 2
    f, bstar = _generate(n, p, seed, s, 1.0, dtype)
    X = f.X_cols(0, p)
    assert X.dtype == dtype
    _check_X(f"small-n{n}", X, seed, 0)
    _check_beta_star(bstar, seed, s)
    _check_y(f"small-n{n}", f, X, bstar, seed, 0, 1.0)
    f.close()


# ---- 2. the grid-stride loops wrap -----------------------------------------------------------------------------------
WRAP = [(n, seed, dt) for n in (2 ** 20 + 3, 2 ** 21 + 5) for seed in SEEDS for dt in DTYPES]


@pytest.mark.parametrize("n,seed,dtype", WRAP, ids=_ids(WRAP))
def test_grid_stride_wrap_every_row(n, seed, dtype):
    p, s = 3, 2
    # cdh_generate's launches, restated: both kernels run out of blocks and go round their loops again
    gx = min(2048, -(-((n + 3) // 2) // 256))
    gy = min(4096, -(-n // 256))
    assert (gx, gy) == (P.gen_x_grid(n)[0], P.gen_y_grid(n)[0])
    assert gx == 2048 and (n + 1) // 2 > gx * 256, "k_gen_X's loop does not wrap at this n"
    assert gy == 4096 and n > gy * 256, "k_gen_y's loop does not wrap at this n"
    x_trip = P.x_trip_of_row(n)
    x_edges = sorted({int(i) for t in range(int(x_trip.max()) + 1) for i in np.nonzero(x_trip == t)[0][[0, -1]]})
    y_edges = sorted({i for t in range(-(-n // (gy * 256))) for i in (t * gy * 256, min(n, (t + 1) * gy * 256) - 1)})
    assert x_trip.max() >= 1 and len(x_edges) >= 4 and len(y_edges) >= 4
    f, bstar = _generate(n, p, seed, s, 1.0, dtype)
    X = f.X_cols(0, p)
    _check_X(f"wrap-n{n}", X, seed, 0, name_rows=x_edges)
    _check_beta_star(bstar, seed, s)
    _check_y(f"wrap-n{n}", f, X, bstar, seed, 0, 1.0, exact_chain=False, name_rows=y_edges)
    f.close()


# ---- 3. the column split ---------------------------------------------------------------------------------------------
SPLIT = [(seed, dt) for seed in SEEDS for dt in DTYPES]


@pytest.mark.parametrize("seed,dtype", SPLIT, ids=_ids(SPLIT))
def test_second_column_slice(seed, dtype):
    n, p, s = 5, P.GEN_COL_SLICE + 3, 2
    assert p > P.GEN_COL_SLICE                              # a second launch of k_gen_X, j0 = 32 768, three blocks along y
    f, bstar = _generate(n, p, seed, s, 1.0, dtype)
    X = f.X_cols(0, p)
    _check_X("colsplit", X, seed, 0, name_cols=(P.GEN_COL_SLICE - 1, P.GEN_COL_SLICE, p - 1))
    _check_y("colsplit", f, X, bstar, seed, 0, 1.0)
    f.close()


# ---- 4. the 64-bit counter -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,dtype", SPLIT, ids=_ids(SPLIT))
def test_counter_high_word(seed, dtype):
    """Rows around global row 2^33 = row pair 2^32, where ctr >> 32 becomes 1; only the shard's 1025 rows exist."""
    n, p, s, n_total = 1025, 3, 2, 2 ** 34
    first = None
    for case, row0 in (("ctr64-straddle", 2 ** 33 - 513), ("ctr64-beyond", 2 ** 33 + 1)):
        assert row0 + n > 2 ** 33 and (case == "ctr64-beyond") == (row0 >= 2 ** 33)
        f, bstar = _generate(n, p, seed, s, 1.0, dtype, n_total=n_total, row_offset=row0)
        X = f.X_cols(0, p)
        _check_X(case, X, seed, row0)
        _check_y(case, f, X, bstar, seed, row0, 1.0)
        _check_beta_star(bstar, seed, s)
        # ... and they are not rows 0.. (nor 1.., the same parity) of the same seed over again
        if first is None:
            f0, _ = _generate(n + 1, p, seed, s, 1.0, dtype)
            first = (f0.X_cols(0, p), f0.y)
            f0.close()
        for shift in (0, 1):
            assert _differ(X, first[0][shift:shift + n])
            assert _differ(f.y, first[1][shift:shift + n])
        f.close()


# ---- 5. shards of one problem, device against device, bit for bit ------------------------------------------------------
@pytest.mark.parametrize("seed,dtype", SPLIT, ids=_ids(SPLIT))
def test_shard_matrix_is_bit_equal_to_the_slice(seed, dtype):
    """A thread owns a global row pair: a shard with odd row_offset starts on the sin member of a pair whose cos member is
    another rank's, one with odd row_offset + n ends on a cos member.  Both parities of both ends, 1 to 513 rows."""
    N, p, s, noise = 4099, 4, 3, 1.5
    whole, bstar = _generate(N, p, seed, s, noise, dtype)
    X, y = whole.X_cols(0, p), whole.y
    whole.close()
    seen = set()
    for a in (0, 1, 2, 511, 512, 513, 4096, 4097):
        for length in (1, 2, 3, 512, 513):
            b = min(N, a + length)
            f, bs = _generate(b - a, p, seed, s, noise, dtype, n_total=N, row_offset=a)
            np.testing.assert_array_equal(f.X_cols(0, p), X[a:b], err_msg=f"rows [{a}, {b})")
            np.testing.assert_array_equal(f.y, y[a:b], err_msg=f"rows [{a}, {b})")
            np.testing.assert_array_equal(f.r, y[a:b], err_msg=f"rows [{a}, {b})")
            np.testing.assert_array_equal(bs, bstar)
            f.close()
            seen.add((a % 2, b % 2))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- 6. k_gen_y --------------------------------------------------------------------------------------------------------
GENY = [(s, seed, dt) for s in (0, 1, 5) for seed in SEEDS for dt in DTYPES]


@pytest.mark.parametrize("s,seed,dtype", GENY, ids=_ids(GENY))
def test_y_is_the_fma_chain_over_the_stored_x(s, seed, dtype):
    n, p = 257, 5                                           # two blocks of k_gen_y; s = 0, 1, p
    f, bstar = _generate(n, p, seed, s, 0.0, dtype)
    assert bstar.shape == (s,)                              # s = 0: empty, and the call succeeded
    X = f.X_cols(0, p)
    _check_X("y-n257", X, seed, 0)
    _check_beta_star(bstar, seed, s)
    _check_y("y-n257-noise0", f, X, bstar, seed, 0, 0.0)    # bit equality
    if s == 0:
        assert not f.y.any()
    status, bstar2 = _regenerate(f, seed, s, 2.5)
    assert status == 0
    np.testing.assert_array_equal(bstar2, bstar)
    np.testing.assert_array_equal(f.X_cols(0, p), X)
    _check_y("y-n257-noise2.5", f, X, bstar, seed, 0, 2.5)
    f.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_s_out_of_range_is_refused_and_the_handle_generates_afterwards(dtype):
    n, p = 257, 5
    f, bstar = _generate(n, p, 123, 2, 1.0, dtype)
    X, y = f.X_cols(0, p), f.y
    for s in (p + 1, -1):
        status, _ = _regenerate(f, 7, s, 1.0)
        assert status == CDH_BAD_ARG
        with pytest.raises(cd.ArgumentError):
            cd._lib.check(status, f._h)
        np.testing.assert_array_equal(f.X_cols(0, p), X)    # refused before anything was written
        np.testing.assert_array_equal(f.y, y)
    status, b7 = _regenerate(f, 7, p, 1.0)
    assert status == 0
    X7 = f.X_cols(0, p)
    _check_X("after-refusal", X7, 7, 0)
    _check_beta_star(b7, 7, p)
    _check_y("after-refusal", f, X7, b7, 7, 0, 1.0)
    f.close()


# ---- 7. pad rows -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("n", [5, 33, 63])
def test_pad_rows_stay_zero_under_the_summing_kernels(cus, n, dtype):
    """Rows [n, ld) of X, y and r are zero by contract (cdh_create), the generator's guards i0 < n, i1 < n keep them so, and
    every summing kernel reads them.  After two generations on one handle, cdh_xt_r and cdh_gram agree with numpy on the
    downloaded X and y within the rounded-data bounds of tests/test_gpu_kernel_sums.py: 4 L 2^-53 |x_k| |r| for the column
    dots (fp64 accumulation for either storage), 4 L 2^-53 sqrt(a_i a_j) for k_gramstep on fp64 storage.  On fp32 storage
    k_gramstep sums up to 256 rows in fp32 before it folds into fp64 (the chain lengths in that file's header), so the n
    <= 63 terms here carry n roundings of 2^-24 on top.  A non-zero pad entry is a term of the order of 1."""
    from test_gpu_kernel_sums import _cdh_gram, col_dots_chunks, gram_grid
    p, s = 6, 2
    ld = -(-n // 32) * 32
    assert ld > n and ld == {5: 32, 33: 64, 63: 64}[n]
    f, _ = _generate(n, p, 123, s, 1.0, dtype)
    status, _ = _regenerate(f, 7, s, 1.0)
    assert status == 0
    X, y = f.X_cols(0, p), f.y
    _check_X(f"pad-n{n}", X, 7, 0)
    XL, yL = X.astype(L), y.astype(L)
    a = np.einsum("ij,ij->j", X.astype(np.float64), X.astype(np.float64))
    yy = float(yL @ yL)
    (chunks,) = col_dots_chunks(n, p, dtype, cus)
    nvec = -(-n // (2 if dtype == np.float64 else 4))
    Lc = -(-nvec // (chunks * 256)) * 2 + 8 + chunks
    out = np.zeros(p)
    cd._lib.check(f._L.cdh_xt_r(f._h, _vp(out)), f._h)
    err = np.abs(out - XL.T @ yL).astype(np.float64) / np.sqrt(a * yy)
    assert err.max() <= 4 * Lc * P.U64, (err.max(), Lc)
    G_blocks, nchunks = gram_grid(n, dtype, cus)
    Lg = -(-nchunks // (4 * G_blocks)) * 128 + 4 + G_blocks
    unit = 4 * Lg * P.U64 + (0.0 if dtype == np.float64 else 4 * n * 2.0 ** -24)
    idx = np.array([1, 3, 4, p])
    G, c, q = _cdh_gram(f, idx)
    errG = np.abs(G - XL[:, idx - 1].T @ XL[:, idx - 1]).astype(np.float64) / np.sqrt(np.outer(a[idx - 1], a[idx - 1]))
    errc = np.abs(c - XL[:, idx - 1].T @ yL).astype(np.float64) / np.sqrt(a[idx - 1] * yy)
    _fig(f"pad-n{n}", dtype=np.dtype(dtype).name, xt_r=err.max(), G=errG.max(), c=errc.max(), unit=unit)
    assert errG.max() <= unit and errc.max() <= unit, (errG.max(), errc.max(), unit)
    assert abs(float(q - yL @ yL)) <= unit * yy
    f.close()


# ---- 8. determinism and seeds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_determinism_seed_words_and_loss_classes(dtype):
    n, p, s = 1027, 7, 3
    f1, b1 = _generate(n, p, 123, s, 1.0, dtype)
    f2, b2 = _generate(n, p, 123, s, 1.0, dtype)
    X1, y1 = f1.X_cols(0, p), f1.y
    assert X1.tobytes() == f2.X_cols(0, p).tobytes() and y1.tobytes() == f2.y.tobytes() and b1.tobytes() == b2.tobytes()
    assert f1.r.tobytes() == f2.r.tobytes()
    f2.close()
    fh, bh = _generate(n, p, 123 + 2 ** 32, s, 1.0, dtype)    # the high word of the seed is Philox's k1
    Xh = fh.X_cols(0, p)
    for j in range(p):
        assert _differ(Xh[:, j], X1[:, j]), f"column {j}: the high 32 bits of the seed do not reach the generator"
    assert _differ(fh.y, y1) and not np.any(bh == b1)
    _check_X("seed-high-word", Xh, 123 + 2 ** 32, 0)
    fh.close()
    classes = [cd.CDSqrtLassoLoss] + ([cd.CDLogisticLoss] if dtype == np.float64 else [])
    for cls in classes:
        g, bg = _generate(n, p, 123, s, 1.0, dtype, cls=cls)
        assert g.X_cols(0, p).tobytes() == X1.tobytes() and g.y.tobytes() == y1.tobytes(), cls.__name__
        assert bg.tobytes() == b1.tobytes()
        g.close()
    f1.close()


# ---- 9. a handle that has already solved -------------------------------------------------------------------------------
ROUTES = ("streamed", "cache", "device_loop", "one_launch")
USED = [(route, dt) for route in ROUTES for dt in DTYPES]


def _route(f, route):
    if route == "streamed":
        f.set_gradient_cache(0)
        f.set_onchip_solve(False)
    elif route in ("cache", "device_loop"):
        f.set_gradient_cache(3)
        f.set_onchip_solve(False)
        f.set_device_loop(route == "device_loop")
    else:
        f.set_onchip_solve(True)


def _route_count(f, route):
    return {"streamed": lambda: 1, "cache": lambda: f.cache_stats()["passes"],
            "device_loop": lambda: f.device_loop_stats()["launches"],
            "one_launch": lambda: f.onchip_stats()["solves"]}[route]()


def _solve_path(f, p):
    x = cd.SparseIterate(p)
    cd.initialize_(f, x)
    lmax = cd.findLambdaMax(x, f, cd.ProxL1(1.0))
    rec = [lmax]
    for frac in (0.5, 0.2, 0.08):
        cd.coordinateDescent_(x, f, cd.ProxL1(frac * lmax), cd.CDOptions(maxIter=300, optTol=1e-7, randomize=False))
        rec.append({"beta": x.dense(), "support": x.nzval2ind.tolist(), "passes": f.last_stats["passes"],
                    "visits": f.last_stats["visits"], "converged": f.last_stats["converged"]})
    rec.append(f.r)
    return rec, x.nnz


def _same_path(got, want):
    """lambda_max, then per lambda the iterate (bit for bit), the support order and the counts, then the residual."""
    assert got[0] == want[0], ("lambda_max", got[0], want[0])
    for i, (g, w) in enumerate(zip(got[1:-1], want[1:-1])):
        for key in ("passes", "visits", "converged", "support"):
            assert g[key] == w[key], (f"lambda {i}", key, g[key], w[key])
        d = np.abs(g["beta"] - w["beta"])
        assert g["beta"].tobytes() == w["beta"].tobytes(), (f"lambda {i}", "beta", int((d > 0).sum()), float(d.max()))
    assert got[-1].tobytes() == want[-1].tobytes(), ("r", float(np.abs(got[-1] - want[-1]).max()))


@pytest.mark.parametrize("route,dtype", USED, ids=_ids(USED))
def test_regenerating_on_a_used_handle_equals_a_fresh_handle(monkeypatch, route, dtype):
    """cdh_generate on a handle that has solved (rs.regenerated, gc_invalidate, yy_void, small_invalidate, x.clear, beta
    zeroed): the data, and a path solved on it afterwards, are those of a new handle -- nothing of the first problem's Gram
    columns, column norms, |y|^2, support or residual bookkeeping survives."""
    if route == "one_launch":
        monkeypatch.setenv("CDH_SMALL_PATH", "1")
    n, p, s = 3000, 40, 5
    fresh, bf = _generate(n, p, 123, s, 1.0, dtype)
    _route(fresh, route)
    used, _ = _generate(n, p, 7, s, 1.0, dtype)
    _route(used, route)
    _, nnz7 = _solve_path(used, p)
    assert nnz7 > 0 and _route_count(used, route) > 0, route
    before = dict(used.cache_stats(), **{k: v for k, v in used.device_loop_stats().items() if isinstance(v, int)})
    status, bu = _regenerate(used, 123, s, 1.0)
    assert status == 0
    np.testing.assert_array_equal(bu, bf)
    assert cd.objective(used) == cd.objective(fresh)
    for name, a, b in (("X", used.X_cols(0, p), fresh.X_cols(0, p)), ("y", used.y, fresh.y), ("r", used.r, fresh.r)):
        assert a.tobytes() == b.tobytes(), name
    beta = np.ones(p)
    cd._lib.check(used._L.cdh_get_beta(used._h, _vp(beta)), used._h)
    assert not beta.any()
    want, nnz = _solve_path(fresh, p)
    got, _ = _solve_path(used, p)
    assert nnz > 0 and _route_count(fresh, route) > 0, route
    after = dict(used.cache_stats(), **{k: v for k, v in used.device_loop_stats().items() if isinstance(v, int)})
    new = dict(fresh.cache_stats(), **{k: v for k, v in fresh.device_loop_stats().items() if isinstance(v, int)})
    _fig(f"used-{route}", dtype=np.dtype(dtype).name, fresh=new, used={k: after[k] - before[k] for k in after})
    _same_path(got, want)
    assert used.X_cols(0, p).tobytes() == fresh.X_cols(0, p).tobytes() and used.y.tobytes() == fresh.y.tobytes()
    used.close()
    fresh.close()
