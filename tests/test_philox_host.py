"""The numpy twin of the problem generator (tests/_philox_numpy.py), checked on the CPU: that it is Philox4x32-10 (the
Random123 known answers), that its uniforms end where the code's comment says, that it is a Gaussian generator with
independent streams, that it shards, and that the comparison tests/test_gpu_generator.py makes between the device and the
twin fails for each of six ways the generator could be wrong -- shown by putting the mistake into a copy of the twin.

Statistical bounds are k / sqrt(N) with k written out next to the standard deviation it is four (or more) of; the seeds
are fixed, so every figure is deterministic.
"""
import math

import numpy as np
import pytest

import _philox_numpy as P

SEEDS = (123, 7)


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
], ids=["zeros", "ones", "pi"])
def test_random123_known_answers(ctr, key, want):
    got = P.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want
    # vectorised: the same words at every position of an array
    got = P.philox4x32_10(*(np.full(3, c, dtype=np.uint64) for c in ctr), *key)
    assert all(w.tolist() == [x] * 3 for w, x in zip(got, want))


def test_uniforms_wire_counter_column_stream_and_both_seed_words():
    """uniforms(seed, ctr, col, stream) is Philox on counter (ctr lo, ctr hi, col, stream), key (seed lo, seed hi); the four
    words feed u1 (words 0, 1) and u2 (words 2, 3)."""
    seed, ctr, col, stream = (0x299f31d0 << 32) | 0xa4093822, (0x85a308d3 << 32) | 0x243f6a88, 0x13198a2e, 0x03707344
    u1, u2 = P.uniforms(seed, ctr, col, stream)
    w = (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    assert u1 == ((w[0] >> 5) * 2 ** 26 + (w[1] >> 6) + 0.5) / 2 ** 53       # (int + 0.5 in Python: the same one fp64
    assert u2 == ((w[2] >> 5) * 2 ** 26 + (w[3] >> 6) + 0.5) / 2 ** 53       # addition, rounded to even)


def test_ends_of_uniforms():
    """(k + 0.5) 2^-53: k = 0 gives 2^-54; k = 2^53 - 1 needs 54 bits, rounds to even and gives exactly 1.0.  The interval is
    (0, 1].  Both ends give a finite normal: log(1) = 0 so rad = 0, and 2^-54 gives rad = sqrt(108 ln 2) < 8.66."""
    lo, hi = float(P.uniform_of_k(0)), float(P.uniform_of_k(2 ** 53 - 1))
    assert lo == 2.0 ** -54 and hi == 1.0
    assert float(P.uniform_of_k(2 ** 52)) == (2.0 ** 52 + 0.0) / 2 ** 53    # 2^52 + 0.5 ties to the even 2^52
    assert float(P.uniform_of_k(2 ** 52 + 1)) == (2.0 ** 52 + 2.0) / 2 ** 53
    assert float(P.uniform_of_k(2 ** 52 - 1)) == (2.0 ** 52 - 0.5) / 2 ** 53  # below 2^52 the half is kept
    for u1 in (lo, hi):
        for u2 in (lo, 0.25, 0.5, hi):
            (c, cL), (s, sL), rad = P.box_muller(u1, u2)
            for val in (float(c), float(s), float(cL), float(sL)):
                assert math.isfinite(val) and abs(val) < P.X_ABS_MAX
            assert (rad == 0.0 and c == 0.0 and s == 0.0) if u1 == hi else abs(float(rad) - math.sqrt(108 * math.log(2))) < 1e-14


# ---- a Gaussian generator ---------------------------------------------------------------------------------------------
N_STAT = 200_000
RN = 1.0 / math.sqrt(N_STAT)


@pytest.fixture(scope="module")
def columns():
    """Per seed: rows [0, N) of X columns 0 and 1 and the noise, fp64 values of the twin."""
    out = {}
    for seed in SEEDS:
        X, _, _ = P.x_matrix(seed, 0, N_STAT, 0, 2)
        e, _, _ = P.noise(seed, np.arange(N_STAT))
        out[seed] = (X, e)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_moments_of_a_column(columns, seed):
    for x in (columns[seed][0][:, 0], columns[seed][1]):
        m, v = x.mean(), x.var()
        z = (x - m) / math.sqrt(v)
        assert abs(m) < 4.0 * RN                          # sd 1/sqrt N: 4 sd
        assert abs(v - 1.0) < 6.0 * RN                    # sd sqrt(2/N): 4.2 sd
        assert abs(np.mean(z ** 3)) < 10.0 * RN           # sd sqrt(6/N): 4.1 sd
        assert abs(np.mean(z ** 4) - 3.0) < 20.0 * RN     # sd sqrt(24/N): 4.1 sd


def _corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize("seed", SEEDS)
def test_members_columns_and_streams_are_uncorrelated(columns, seed):
    X, e = columns[seed]
    k = 4.0                                                 # each sample correlation has sd 1/sqrt(its N)
    assert abs(_corr(X[0::2, 0], X[1::2, 0])) < k / math.sqrt(N_STAT // 2)   # the cos and sin members of a pair
    assert abs(_corr(X[:, 0], X[:, 1])) < k * RN            # adjacent columns
    assert abs(_corr(X[:, 0], e)) < k * RN                  # X column 0 and the noise: the same (pair, col 0), another stream
    assert abs(_corr(X[:-1, 0], X[1:, 0])) < k * RN         # adjacent rows, within pairs and across them


@pytest.mark.parametrize("seed", SEEDS)
def test_tail_share_beyond_three_sigma(columns, seed):
    q = math.erfc(3.0 / math.sqrt(2.0))                     # 0.0027; the share has sd sqrt(q (1 - q) / N) = 0.052 / sqrt N
    share = float(np.mean(np.abs(columns[seed][0][:, 0]) > 3.0))
    assert abs(share - q) < 0.25 * RN                       # 4.8 sd
    assert np.abs(columns[seed][0]).max() < P.X_ABS_MAX


def test_streams_are_disjoint_counters():
    """X (stream 0), the noise (stream 1) and beta* (stream 2) of the same (pair, column 0) share no uniform."""
    ctr = np.arange(64)
    u = [np.concatenate(P.uniforms(123, ctr, 0, st)) for st in (P.STREAM_X, P.STREAM_NOISE, P.STREAM_BETA)]
    assert len(set(np.concatenate(u).tolist())) == 3 * 128
    b, bL, scale = P.beta_star(123, 5)
    z, _, _ = P.normal(123, 2 * np.arange(5), 0, P.STREAM_BETA)
    u1, _ = P.uniforms(123, np.arange(5), 1, P.STREAM_BETA)
    np.testing.assert_array_equal(b, z * (1.0 + u1))
    assert np.all(np.abs(b - bL).astype(np.float64) <= P.ULPS * P.U64 * scale)
    assert P.beta_star(123, 0)[0].shape == (0,)


# ---- sharding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(0, 1), (1, 2), (0, 7), (1, 7), (1, 8), (2, 8), (510, 1023), (511, 1024), (33, 34), (34, 35)])
def test_a_shard_of_the_twin_is_that_slice(a, b):
    N, p = 1025, 3
    full = P.x_matrix(123, 0, N, 0, p)
    part = P.x_matrix(123, a, b - a, 0, p)
    entry = P.x_entry(123, np.arange(a, b)[:, None], np.arange(p)[None, :])
    for f, s, e in zip(full, part, entry):
        np.testing.assert_array_equal(s, f[a:b])
        np.testing.assert_array_equal(e, f[a:b])
    ef, es = P.noise(123, np.arange(N)), P.noise(123, np.arange(a, b))
    np.testing.assert_array_equal(es[0], ef[0][a:b])
    for whole, part in zip(ef, P.noise_vector(123, a, b - a)):
        np.testing.assert_array_equal(part, whole[a:b])


def test_seed_high_word_reaches_the_key():
    a, _, _ = P.x_matrix(123, 0, 512, 0, 4)
    b, _, _ = P.x_matrix(123 + 2 ** 32, 0, 512, 0, 4)
    assert not np.any(a == b)
    assert not np.any(P.noise(123, np.arange(512))[0] == P.noise(123 + 2 ** 32, np.arange(512))[0])
    assert not np.any(P.beta_star(123, 16)[0] == P.beta_star(123 + 2 ** 32, 16)[0])


# ---- y ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("s", [0, 1, 5])
def test_y_exact_against_a_longdouble_dot(dtype, s):
    """The fma chain rounds once per term: |chain - exact dot| <= s 2^-53 sum |x_j b_j|."""
    n = 257
    X = P.x_matrix(7, 0, n, 0, 5)[0].astype(dtype)
    b = P.beta_star(7, s)[0]
    y = P.y_exact(X[:, :s], b)
    L = np.longdouble
    dot = (X[:, :s].astype(L) * b.astype(L)).sum(axis=1)
    bound = s * P.U64 * (np.abs(X[:, :s].astype(np.float64)) * np.abs(b)).sum(axis=1)
    assert np.all(np.abs(y.astype(L) - dot).astype(np.float64) <= bound)
    if s == 0:
        assert not y.any()
    if s == 1:
        np.testing.assert_array_equal(y, X[:, 0].astype(np.float64) * b[0])
    e = np.arange(n, dtype=np.float64)
    np.testing.assert_array_equal(P.y_exact(X[:, :s], b, e), y + e)


def test_fma_is_rounded_once():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30               # a b = 1 - 2^-60: the product alone rounds to 1
    assert a * b - 1.0 == 0.0 and P._fma(a, b, -1.0) == -2.0 ** -60


# ---- the launch arithmetic --------------------------------------------------------------------------------------------
def test_restated_grids():
    assert P.gen_x_grid(1) == (1, 256) and P.gen_x_grid(512) == (2, 512) and P.gen_x_grid(509) == (1, 256)
    assert P.gen_x_grid(2 ** 20 - 3) == (2048, 2 ** 19) and P.gen_x_grid(2 ** 24) == (2048, 2 ** 19)
    assert P.gen_y_grid(1) == (1, 256) and P.gen_y_grid(257) == (2, 512) and P.gen_y_grid(2 ** 22) == (4096, 2 ** 20)
    t = P.x_trip_of_row(2 ** 20 + 3)
    assert t.max() == 1 and int(np.argmax(t)) == 2 ** 20 and np.all(np.diff(t) >= 0)
    t = P.x_trip_of_row(2 ** 20 + 3, row0=1)                # the pair of row0 - 1 and row0 is pair 0 of the shard
    assert int(np.argmax(t)) == 2 ** 20 - 1


# ---- fp32: the boundary exceptions stay under the cap for the shapes and seeds of the GPU test --------------------------
def test_f32_expected_admits_the_neighbour_only_at_a_boundary():
    L = np.longdouble
    f = np.float32(1.5)
    up = np.nextafter(f, np.float32(2))
    mid = (L(f) + L(up)) / 2
    tol = L(P.ULPS * P.U64 * 2.0)                            # rad = 2
    ref = np.array([mid - tol, mid + tol, mid - 3 * tol, L(f)], dtype=L)
    got, alt, near = P.f32_expected(ref, np.full(4, 2.0))
    assert got.tolist() == [f, up, f, f] and alt.tolist() == [up, f, f, f] and near.tolist() == [True, True, False, False]


def _case_blocks():
    """(name, seed, row0, n, col0, p) of every block of X the GPU test compares with the twin in fp32."""
    out = []
    for seed in SEEDS:
        for n in (1, 2, 3, 31, 32, 33, 511, 512, 513):
            out.append((f"small-n{n}", seed, 0, n, 0, 5))
        out.append(("colsplit", seed, 0, 5, 0, 32768 + 3))
        out.append(("ctr64-straddle", seed, 2 ** 33 - 513, 1025, 0, 3))
        out.append(("ctr64-beyond", seed, 2 ** 33 + 1, 1025, 0, 3))
        out.append(("y-n257", seed, 0, 257, 0, 5))
        for n in (2 ** 20 + 3, 2 ** 21 + 5):
            out.append((f"wrap-n{n}", seed, 0, n, 0, 3))
    return out


@pytest.mark.parametrize("name,seed,row0,n,col0,p", _case_blocks(), ids=[f"{c[0]}-seed{c[1]}" for c in _case_blocks()])
def test_f32_boundary_exceptions_stay_under_the_cap(name, seed, row0, n, col0, p):
    """About ULPS 2^-53 rad / (2^-24 |x|) ~ 1e-8 of the entries lie that close to an fp32 rounding boundary; the GPU test
    caps the share at 1e-6 of a case (no exception at all in a case of fewer than 10^6 entries).  The twin's own fp64 values
    pass the fp32 comparison too."""
    x, ref, rad = P.x_matrix(seed, row0, n, col0, p)
    f, alt, near = P.f32_expected(ref, rad)
    assert int(near.sum()) <= P.F32_EXCEPTION_SHARE * near.size, (int(near.sum()), near.size)
    bad, fig = P.check_x(x.astype(np.float32), ref, rad)
    assert not bad.any(), fig
    bad, fig = P.check_x(x, ref, rad)
    assert not bad.any() and fig["max_err_in_2^-53_rad"] < 4.0, fig     # numpy's own math library: 2.6 on x86-64 glibc


# ---- teeth: six ways to be wrong, each put into a copy of the twin, each caught by the GPU test's comparison ------------
def _cut_to_one_trip(X, n, row0=0):
    """What k_gen_X leaves if its grid-stride loop makes one trip: the rows of later trips keep the zeros of cdh_create."""
    X = X.copy()
    X[P.x_trip_of_row(n, row0) > 0] = 0.0
    return X


MISTAKES = {
    # name: (the twin with the mistake, (row0, n, col0, p) of the GPU case that must catch it)
    "philox_multiplier": (P.Variant(m0=P.PHILOX_M0 ^ 0x100), (0, 33, 0, 5)),
    "nine_rounds": (P.Variant(rounds=9), (0, 33, 0, 5)),
    "cos_sin_swapped": (P.Variant(swap=True), (0, 33, 0, 5)),
    "one_trip_of_the_stride_loop": (None, (0, 2 ** 20 + 3, 0, 1)),
    "col_modulo_32768": (P.Variant(col_mask=32768), (0, 5, 32760, 11)),
    "ctr_high_word_dropped": (P.Variant(drop_ctr_hi=True), (2 ** 33 - 513, 1025, 0, 3)),
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_each_mistake_fails_the_comparison_the_gpu_test_makes(mistake, dtype):
    variant, (row0, n, col0, p) = MISTAKES[mistake]
    good, ref, rad = P.x_matrix(7, row0, n, col0, p)
    bad_mask, _ = P.check_x(good.astype(dtype), ref, rad)
    assert not bad_mask.any()                                 # the unperturbed copy passes
    if variant is None:
        wrong = _cut_to_one_trip(good, n, row0)
    else:
        wrong, _, _ = P.x_matrix(7, row0, n, col0, p, variant)
    bad_mask, _ = P.check_x(wrong.astype(dtype), ref, rad)
    assert bad_mask.any()
    rows, cols = np.nonzero(bad_mask)
    if mistake == "one_trip_of_the_stride_loop":
        assert rows.min() == 2 ** 20 and rows.max() == n - 1    # exactly the rows of the second trip
    elif mistake == "col_modulo_32768":
        assert cols.min() == 32768 - col0                     # the first slice is right, the second repeats it
    elif mistake == "ctr_high_word_dropped":
        assert rows.min() == 513                              # local row 513 is global row 2^33
    elif mistake == "cos_sin_swapped":
        np.testing.assert_array_equal(wrong[0:32:2], good[1:33:2])
        assert bad_mask.mean() > 0.9
    else:
        assert bad_mask.mean() > 0.9                          # another stream altogether
    # the noise and beta* of the same mistake (they share struct Philox with X)
    if variant is not None and mistake not in ("col_modulo_32768",):
        rows_g = row0 + np.arange(n)
        e, eL, erad = P.noise(7, rows_g)
        ew, _, _ = P.noise(7, rows_g, variant)
        assert P.check_x(ew.astype(dtype), eL, erad)[0].any() and not P.check_x(e.astype(dtype), eL, erad)[0].any()
