"""The numpy twin of Harrell's concordance index (csrc/cox_concordance.hip; cdh_glm_cox_concordance), in two halves that
tests/test_cox_concordance_host.py holds equal with ==.

`definition` is the O(n^2) statement: rows i != j that take part, in one stratum, are a comparable pair with i the earlier iff i
is an event and t_j > t_i, or t_j == t_i and j is censored; the pair is concordant if eta_i > eta_j, discordant if eta_i < eta_j,
tied if they are equal (doubles: -0.0 == 0.0), and counts v_i v_j.

`levels` is what the device runs, level by level: the concordance order (`conc_order`, the restatement of cox_plan.hpp's
cox_conc_order), a bottom-up merge sort of eta over its positions, and for every event the at most two whole runs per level that
tile its range [qa, qb) (`take`, cox_conc_take), in which the weight of the smaller eta is the run's prefix sum at the event's
lower-bound rank, that of the smaller-or-equal its prefix sum at the upper-bound rank, and the run's total its last prefix sum.
Rows outside the subset carry the key +inf and the weight 0.  `levels_vectorised` is the same walk with every level's queries
answered at once (what tools/cox_concordance_timing.py times as the host-composed alternative).  The twin walks ALL levels
from 0; the device counts the levels below its tile position by position (`fringe`, cox_conc_fringe), which is the same set of
rows.

dtype=np.longdouble runs either half's sums in long double (the reference of the weighted tests)."""
import numpy as np

TILE = 1024          # kCoxTile
TILE_LOG = 10        # kCoxTileLog


def cindex(c, d, t):
    tot = c + d + t
    return float((c + t / 2) / tot) if tot > 0 else float("nan")


def definition(time, status, eta, strata=None, weights=None, subset=None, dtype=np.float64):
    """-> (concordant, discordant, tied) by the definition, every pair looked at; sums in dtype, rows in order."""
    time, status, eta = (np.asarray(a, dtype=np.float64) for a in (time, status, eta))
    n = len(time)
    g = np.zeros(n, dtype=np.int64) if strata is None else np.asarray(strata)
    v = np.ones(n, dtype=dtype) if weights is None else np.asarray(weights).astype(dtype)
    R = np.ones(n, dtype=bool) if subset is None else np.asarray(subset, dtype=bool)
    c = d = t = dtype(0)
    for i in range(n):
        if not (R[i] and status[i] == 1.0):
            continue
        later = R & (g == g[i]) & ((time > time[i]) | ((time == time[i]) & (status == 0.0)))
        later[i] = False
        c += v[i] * np.sum(v[later & (eta < eta[i])], dtype=dtype)
        d += v[i] * np.sum(v[later & (eta > eta[i])], dtype=dtype)
        t += v[i] * np.sum(v[later & (eta == eta[i])], dtype=dtype)
    return c, d, t


def conc_order(time, status, strata=None, ld=None, N=None):
    """-> (corder, qa, qb), N entries each (ld, N default n): a stable sort by (stratum, time, events before censored); for an
    event position its range of comparable positions -- from the first censored position of its tie group (the group's end
    without one) to the end of its stratum; qa = qb = 0 elsewhere.  Pads n .. ld - 1 stay in place; beyond ld the row is -1."""
    time, status = np.asarray(time, dtype=np.float64), np.asarray(status, dtype=np.float64)
    n = len(time)
    ld = n if ld is None else ld
    N = ld if N is None else N
    g = np.zeros(n, dtype=np.int64) if strata is None else np.asarray(strata, dtype=np.int64)
    rows = np.lexsort((np.arange(n), status != 1.0, time, g))          # the last key is the primary one
    corder = np.full(N, -1, dtype=np.int32)
    corder[:n] = rows
    corder[n:ld] = np.arange(n, ld)
    qa, qb = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    if n:
        gs, ts, event = g[rows], time[rows], status[rows] == 1.0
        new_stratum = np.r_[True, gs[1:] != gs[:-1]]
        new_group = new_stratum | np.r_[True, ts[1:] != ts[:-1]]
        starts, sstarts = np.nonzero(new_group)[0], np.nonzero(new_stratum)[0]
        gid, sid = np.cumsum(new_group) - 1, np.cumsum(new_stratum) - 1
        censored = starts + np.add.reduceat(event.astype(np.int64), starts)    # the group's first censored position, or its end
        ends = np.r_[sstarts[1:], n]
        qa[:n] = np.where(event, censored[gid], 0)
        qb[:n] = np.where(event, ends[sid], 0)
    return corder, qa, qb


def take(a, b, lev):
    """The runs of level lev that the walk over [a, b) takes: at most two, whole."""
    l, r = -((-a) >> lev), b >> lev
    runs = []
    if l < r:
        if l & 1:
            runs.append(l)
        if r & 1:
            runs.append(r - 1)
    return runs


def fringe(a, b, tile=TILE):
    """-> (a1, b0): the levels below the tile take [a, a1) and [b0, b), the levels from the tile's up tile [a1, b0)."""
    a1 = min(-(-a // tile) * tile, b)
    b0 = max(b // tile * tile, a1)
    return a1, b0


def levels(time, status, eta, strata=None, weights=None, subset=None, dtype=np.float64):
    """-> (concordant, discordant, tied) read off the levels of a bottom-up merge sort, nothing cached."""
    time, status, eta = (np.asarray(a, dtype=np.float64) for a in (time, status, eta))
    n = len(time)
    corder, qa, qb = conc_order(time, status, strata)
    v = np.ones(n, dtype=dtype) if weights is None else np.asarray(weights).astype(dtype)
    R = np.ones(n, dtype=bool) if subset is None else np.asarray(subset, dtype=bool)
    key0 = np.where(R[corder], eta[corder], np.inf)
    v0 = np.where(R[corder], v[corder], dtype(0)).astype(dtype)
    asks = (v0 > 0) & (qa < qb)
    L, E, G = (np.zeros(n, dtype=dtype) for _ in range(3))
    keys, vals = key0.copy(), v0.copy()
    lev = 0
    while True:
        size = 1 << lev
        pre = np.zeros(n, dtype=dtype)
        for b0 in range(0, n, size):                      # the inclusive prefix sums inside the runs
            pre[b0:b0 + size] = np.cumsum(vals[b0:b0 + size], dtype=dtype)
        for s in np.nonzero(asks)[0]:
            for m in take(int(qa[s]), int(qb[s]), lev):
                run = keys[m * size:(m + 1) * size]
                lo, up = np.searchsorted(run, key0[s], "left"), np.searchsorted(run, key0[s], "right")
                L[s] += pre[m * size + lo - 1] if lo else 0
                E[s] += pre[m * size + up - 1] if up else 0
                G[s] += pre[m * size + size - 1]
        if size >= n:
            break
        for b0 in range(0, n, 2 * size):                  # the next level: a stable merge of the sibling runs
            idx = b0 + np.argsort(keys[b0:b0 + 2 * size], kind="stable")
            keys[b0:b0 + 2 * size], vals[b0:b0 + 2 * size] = keys[idx], vals[idx]
        lev += 1
    c = np.sum(v0 * L, dtype=dtype)
    t = np.sum(v0 * (E - L), dtype=dtype)
    d = np.sum(v0 * (G - E), dtype=dtype)
    return c, d, t


def levels_vectorised(time, status, eta, strata=None, weights=None, subset=None, dtype=np.float64):
    """`levels` without a Python loop over the rows: the positions padded to a power of two, eta replaced by its dense rank, a
    level's runs the rows of a matrix sorted along axis 1, and all queries of a level one searchsorted on (run, rank)."""
    time, status, eta = (np.asarray(a, dtype=np.float64) for a in (time, status, eta))
    n = len(time)
    P = 1
    while P < n:
        P *= 2
    corder, qa, qb = conc_order(time, status, strata)
    v = np.ones(n, dtype=dtype) if weights is None else np.asarray(weights).astype(dtype)
    R = np.ones(n, dtype=bool) if subset is None else np.asarray(subset, dtype=bool)
    key0 = np.full(P, np.inf)
    key0[:n] = np.where(R[corder], eta[corder], np.inf)
    v0 = np.zeros(P, dtype=dtype)
    v0[:n] = np.where(R[corder], v[corder], dtype(0))
    _, rank = np.unique(key0, return_inverse=True)                    # equal eta (-0.0 and 0.0 too) share a rank
    rank = rank.astype(np.int64).ravel()
    top = int(rank.max()) + 1
    ev = np.nonzero((v0[:n] > 0) & (qa < qb))[0]
    a, b, x = qa[ev].astype(np.int64), qb[ev].astype(np.int64), rank[ev]
    L, E, G = (np.zeros(len(ev), dtype=dtype) for _ in range(3))
    lev = 0
    while True:
        size = 1 << lev
        by_run = rank.reshape(-1, size)
        idx = np.argsort(by_run, axis=1, kind="stable")
        keys = (np.take_along_axis(by_run, idx, axis=1) + (np.arange(P // size, dtype=np.int64) * top)[:, None]).ravel()
        pre = np.cumsum(np.take_along_axis(v0.reshape(-1, size), idx, axis=1), axis=1, dtype=dtype).ravel()
        l, r = -((-a) >> lev), b >> lev
        for m, on in ((l, (l < r) & (l & 1 == 1)), (r - 1, (l < r) & (r & 1 == 1))):
            m, xs = m[on], x[on]
            lo = np.searchsorted(keys, m * top + xs, "left")
            up = np.searchsorted(keys, m * top + xs, "right")
            L[on] += np.where(lo > m * size, pre[np.maximum(lo - 1, 0)], 0)
            E[on] += np.where(up > m * size, pre[np.maximum(up - 1, 0)], 0)
            G[on] += pre[(m + 1) * size - 1]
        if size >= P:
            break
        lev += 1
    w = v0[ev]
    return np.sum(w * L, dtype=dtype), np.sum(w * (G - E), dtype=dtype), np.sum(w * (E - L), dtype=dtype)
