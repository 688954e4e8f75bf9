"""The cases of tests/test_gpu_cox_runs.py, without the device: the three shapes at which k_cox_offsets -- the scan over the
runs' records, the third level of the Cox step's chain of scans -- leaves one lane, one wave and runs at the full grid; the
strata arrangements and closed forms of its exact leg; the random problems of its wide-twin leg; and the asserts that say, by
tests/_cox_plan.py's arithmetic alone, that each case is the shape it is there for.  tests/test_cox_wide_host.py runs every
assert here without a GPU, so the bookkeeping fails there before it fails on the card.

Shapes (T = 1024 positions a tile, full grid of at most 1024 runs; a lane of k_cox_offsets holds 4 runs, a wave 256):
    R6     n = 5T + 3      6 tiles, 6 runs: the offsets scan leaves one lane's four slots, so `base` is not 0
    R301   n = 300T + 7    301 tiles, 301 runs: it crosses a wave (s_w, s_f), and the last lane's chunk is partial (75 4 + 1)
    R1024  n = 1535T + 5   1536 tiles, 1024 runs of one and two tiles in turn (run b starts at tile floor(3b / 2)): all four
                           waves, a carry from tile to tile inside a run, 1024 records into k_gram_reduce

The exact leg.  Empty iterate, no offset, unit weights: eta = 0, ev = 1.  A stratum of m rows (m a power of two) has stop
times 1 .. m and ONE event, the row with stop 1: S = m there, so A = 1 / m and B = 1 / m^2 on every row -- sums of one term,
exact whatever the order of the additions (the other terms are zeros).  w = 1/m - 1/m^2 is exact (m <= 8192 needs 26 bits), and
above wmin = 1e-5 for every m >= 2; m = 1 has w_raw = 0 and clamps.  r = (delta - A) / w is one IEEE division and z = r.
A "late" stratum (interval chain, m >= 2): the m / 2 rows with the largest stops start at 1, the event's time, so they are not at
risk at it: S = m / 2, and the early rows have A = 2 / m, B = 4 / m^2.  A late row's `enter` is the event's position, so its
A = P[last] - P[enter] is the difference of two prefix sums that hold the same single term: 0 exactly, w = wmin, r = 0.
A late stratum of 2 rows clamps on both (w_raw = 1 - 1 and 0).  Any error in a head flag, a run's offset or a carry makes
some S, A or B another number, and the comparison is ==."""
import numpy as np

import _cox_plan as CP

T = CP.TILE
SHAPES = {"R6": 5 * T + 3, "R301": 300 * T + 7, "R1024": 1535 * T + 5}
RUNS = {"R6": 6, "R301": 301, "R1024": 1024}
PRESORTED = {"R6": False, "R301": True, "R1024": False}
WMIN, EMAX = 1e-5, 1.5


def run_edges(n):
    """The first sorted position of every run and, last, ld: grid + 1 numbers."""
    ld = CP.padded(n)
    pl = CP.plan(ld)
    return np.array([min(CP.run_first(pl["tiles"], pl["grid"], b) * T, ld) for b in range(pl["grid"] + 1)], dtype=np.int64)


def assert_shape(name):
    """The number of runs; R1024 has runs of one tile and of two, in turn from tile 0: 0, 1, 3, 4, ..., 1534, 1536."""
    n = SHAPES[name]
    pl = CP.plan(CP.padded(n))
    edges = run_edges(n)
    assert pl["grid"] == RUNS[name] and len(edges) == RUNS[name] + 1 and edges[0] == 0 and edges[-1] == CP.padded(n)
    tiles = -(-np.diff(edges) // T)
    if name == "R1024":
        assert pl["tiles"] == 1536 and pl["longest"] == 2
        firsts = [CP.run_first(1536, 1024, b) for b in range(1025)]
        assert firsts[:4] == [0, 1, 3, 4] and firsts[-2:] == [1534, 1536] and firsts == [3 * b // 2 for b in range(1025)]
        assert tiles.tolist() == [1, 2] * 512
    else:
        assert pl["tiles"] == RUNS[name] and np.all(tiles == 1)
    assert RUNS[name] > 4                                        # more runs than one lane of k_cox_offsets holds
    assert (RUNS[name] > 256) == (name != "R6") and (RUNS[name] % 4 == 1) == (name == "R301")
    return edges


def run_flags(n, sfirst, slast):
    """The head flags the kernels write per run, from the strata's bounds per sorted position (the pads n .. ld - 1 are a
    stratum of their own): suffix -- the stratum of the run's first position ends inside the run (k_cox_exp, k_cox_gather);
    prefix -- the stratum of its last position starts inside it (k_cox_hazard)."""
    ld = CP.padded(n)
    sf = np.r_[sfirst, np.full(ld - n, n)]
    sl = np.r_[slast, np.full(ld - n, ld - 1)]
    edges = run_edges(n)
    r0, r1 = edges[:-1], edges[1:]
    return sl[r0] < r1, sf[r1 - 1] >= r0


# ---- the exact leg ---------------------------------------------------------------------------------------------------------------
def exact_sizes(name):
    """R301, R1024: ladders 8192, 4096, ..., 2, 1, 1 (16 tiles each) while they fit, then the rest in binary, largest first.
    R6: small strata fill positions 0 .. 514, ONE stratum of 4096 runs from 515 in run 0 to 4610 in run 4 -- runs 0 to 3 sit in
    one lane of k_cox_offsets and runs 4, 5 in the next, so its sums reach across the two through `base` -- and one of 512
    from 4611 to the end, in run 5: a head INSIDE the second lane's chunk, after which `base` must not be added."""
    n = SHAPES[name]
    if name == "R6":
        sizes = [256 >> k for k in range(9)] + [1, 2, 1, 4096, 512]
    else:
        ladder = [8192 >> k for k in range(14)] + [1]
        assert sum(ladder) == 16 * T
        sizes = ladder * (n // (16 * T))
        rest = n - sum(sizes)
        sizes += [1 << k for k in range(rest.bit_length() - 1, -1, -1) if rest >> k & 1]
    assert sum(sizes) == n and all(s & (s - 1) == 0 and 1 <= s <= 8192 for s in sizes)
    return sizes


def assert_exact_arrangement(name, sizes):
    """Where the strata's boundaries lie against the runs: each property at the shapes it is wanted at."""
    n = SHAPES[name]
    edges = assert_shape(name)
    ends = np.cumsum(sizes)
    bounds = ends[:-1]                                           # the first positions of the strata after the first
    sfirst, slast = np.repeat(ends - sizes, sizes), np.repeat(ends - 1, sizes)
    inner = edges[1:-1]
    on_edge = np.intersect1d(bounds, inner)
    suffix, prefix = run_flags(n, sfirst, slast)
    if name == "R6":
        # one stratum from run 0 into run 4, across the lanes of the offsets scan: runs 1 to 3 have no head in either direction
        assert sfirst[edges[4]] < edges[1] and edges[4] < slast[edges[4]] < edges[5] - 1
        assert not suffix[1:4].any() and not prefix[1:4].any()
        # and the next one from run 4 into run 5: a head in the first slot of the second lane, prefix and suffix
        assert prefix[4] and suffix[4] and sfirst[n - 1] == slast[edges[4]] + 1 and sfirst[edges[5]] == sfirst[n - 1]
    else:
        assert len(on_edge) > 0                                  # a boundary exactly on a run's edge
    if name == "R1024":
        assert np.any(~suffix & ~prefix)                         # a run without a boundary: its flag is 0 in both directions
        inside = np.setdiff1d(bounds, edges)
        assert np.histogram(inside, bins=edges)[0].max() >= 3    # a run with three boundaries or more inside it
        assert any(edges[b] in bounds for b in (256, 512, 768))  # a boundary on the edge between two waves of the offsets scan
        spans = np.searchsorted(edges, ends - 1, side="right") - np.searchsorted(edges, ends - sizes, side="right")
        assert spans.max() >= 2 and max(sizes) >= 4096           # a stratum in three runs or more
        assert np.any(bounds % 4 == 2)                           # a boundary inside a lane's four positions
    return bounds


def exact_problem(sizes, late_s, order):
    """The strata `sizes` in sorted order, late where late_s says (all False: the strata chain), rows permuted by `order`.
    -> dict: time (stop), start (None without a late stratum), status, g, and the closed forms S, A, B, w, r (= z), clamped
    per row, out2 (rows clamped), out4 (events) and S_event (per event, for the nll)."""
    sizes, late_s = np.asarray(sizes), np.asarray(late_s, dtype=bool)
    n, k = int(sizes.sum()), len(sizes)
    assert not np.any(late_s & (sizes < 2))
    ids = 7 * np.arange(k) - 3 * k                               # spread, and negative below 3 k / 7
    first = np.repeat(np.cumsum(sizes) - sizes, sizes)
    m = np.repeat(sizes, sizes).astype(np.float64)
    late = np.repeat(late_s, sizes)
    stop = (np.arange(n) - first + 1).astype(np.float64)        # sorted layout: 1 .. m inside every stratum
    status = (stop == 1.0).astype(np.float64)
    late_row = late & (stop > m / 2)
    start = np.where(late_row, 1.0, 0.0)
    eff = np.where(late, m / 2, m)                               # S at the event
    S = np.where(status == 1.0, eff, m - stop + 1.0)             # later times: everybody has entered
    A = np.where(late_row, 0.0, 1.0 / eff)
    B = np.where(late_row, 0.0, (1.0 / eff) * (1.0 / eff))
    w_raw = A - B
    clamped = ~(w_raw >= WMIN)
    w = np.where(clamped, WMIN, w_raw)
    r = (status - A) / w
    assert np.array_equal(clamped, (eff == 1.0) | late_row)      # only S = 1 and the late rows clamp
    g = np.repeat(ids, sizes)
    o = order
    case = dict(time=stop[o], start=start[o] if late_s.any() else None, status=status[o], g=g[o], S=S[o], A=A[o], B=B[o], w=w[o],
                r=r[o], clamped=clamped[o], late_row=late_row[o], m=m[o], out2=int(clamped.sum()), out4=k,
                S_event=eff[status == 1.0], sizes=sizes, late_strata=late_s)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


_EXACT = {}


def exact_case(name, interval):
    """exact_problem at a shape's arrangement.  In the interval chain every second stratum of each size from 2 up is late, so
    every size is there early and late; at R6, where most sizes come once, every second stratum is, the one of 4096 among
    them (it is early in the strata chain): its T2 is read 2048 positions in, two runs and a lane from where it ends.  Rows in random order, or PRESORTED by stratum and time.  Computed once."""
    key = (name, interval)
    if key in _EXACT:
        return _EXACT[key]
    n = SHAPES[name]
    sizes = np.array(exact_sizes(name))
    assert_exact_arrangement(name, sizes.tolist())
    late_s = np.zeros(len(sizes), dtype=bool)
    if interval and name == "R6":
        late_s = (np.arange(len(sizes)) % 2 == 0) & (sizes >= 2)
        assert 4096 in sizes[late_s] and 512 in sizes[~late_s] and 2 in sizes[~late_s] and late_s.sum() == 6
    elif interval:
        for s in np.unique(sizes[sizes >= 2]):
            late_s[np.nonzero(sizes == s)[0][1::2]] = True
        assert set(sizes[late_s]) == set(sizes[sizes >= 2]) == set(sizes[~late_s & (sizes >= 2)])
    rng = np.random.default_rng(5000 + n + interval)
    _EXACT[key] = exact_problem(sizes, late_s, np.arange(n) if PRESORTED[name] else rng.permutation(n))
    return _EXACT[key]


# ---- the wide-twin leg -----------------------------------------------------------------------------------------------------------
def random_sizes(n, rng):
    """Sizes 2^k, k = 0 .. 13 drawn at random, until n is passed; what is left of n in binary."""
    sizes = []
    while True:
        s = 1 << int(rng.integers(0, 14))
        if sum(sizes) + s > n:
            break
        sizes.append(s)
    rest = n - sum(sizes)
    sizes += [1 << k for k in range(rest.bit_length() - 1, -1, -1) if rest >> k & 1]
    assert sum(sizes) == n
    return sizes


_RANDOM = {}


def random_case(name, chain):
    """chain "plain": X (n x 2), times rounded to a decimal, status, an offset.  "strata": strata ids and weights uniform in
    [0.25, 4] too.  "interval": the recipe of _cox_interval_numpy.make_data (rounded: starts coincide with event times, three
    in ten are 0) with the same strata and weights.  -> dict X, start, time, status, off, g, v; computed once, left unchanged."""
    key = (name, chain)
    if key in _RANDOM:
        return _RANDOM[key]
    import _cox_interval_numpy as CI
    n = SHAPES[name]
    seed = 6000 + n + 7 * len(chain)
    rng = np.random.default_rng(seed)
    start = g = v = None
    if chain == "interval":
        X, start, t, status, off = CI.make_data(n, 2, seed + 1, rounded=True, zero=0.3)
    else:
        X = np.asfortranarray(rng.standard_normal((n, 2)))
        t = np.round(rng.exponential(1.0, n), 1)
        status = (rng.random(n) < 0.7).astype(np.float64)
        off = rng.uniform(-0.5, 0.5, n)
    if chain != "plain":
        sizes = random_sizes(n, rng)
        g = np.repeat(5 * np.arange(len(sizes)) - 2 * len(sizes), sizes)[rng.permutation(n)]
        v = rng.uniform(0.25, 4.0, n)
    if PRESORTED[name]:
        o = np.lexsort((t, g)) if g is not None else np.argsort(t, kind="stable")
        X, t, status, off = np.asfortranarray(X[o]), t[o], status[o], off[o]
        start, g, v = (None if a is None else a[o] for a in (start, g, v))
    case = dict(X=X, start=start, time=t, status=status, off=off, g=g, v=v)
    for a in case.values():
        if a is not None:
            a.setflags(write=False)
    _RANDOM[key] = case
    return case


def assert_random_arrangement(name, chain, first, sfirst, slast):
    """Tie groups (first: per sorted position the first position of its group) straddle run edges; with strata, R1024 holds
    1000 to 2000 of them, runs without a boundary and runs with several."""
    n = SHAPES[name]
    edges = assert_shape(name)
    inner = edges[1:-1]
    inner = inner[inner < n]
    assert np.any(first[inner] < inner)                          # a tie group lies on both sides of a run's edge
    if chain != "plain":
        suffix, prefix = run_flags(n, sfirst, slast)
        assert suffix.any() and prefix.any()
        if name != "R6":
            assert np.any(~suffix & ~prefix) and np.any(np.diff(sfirst) != 0)
        if name == "R1024":
            assert 1000 <= len(np.unique(sfirst)) <= 2000


def held_stretch(name):
    """Sorted positions to hold out beside fold 1: run 511 of R1024 -- two tiles, the last run of the offsets scan's second
    wave -- and five positions on either side: a stretch of e = 0 longer than a run, across two run edges."""
    edges = assert_shape(name)
    a, b = int(edges[511]) - 5, int(edges[512]) + 5
    assert name == "R1024" and edges[512] - edges[511] == 2 * T and b - a > 2 * T
    return a, b
