"""The launches of a cdh_gram / cdh_gram_weighted call and of a varying-coefficient point, restated in Python from gram_block and
vc_point as they stood in cdhip.hip before csrc/stats_plan.hpp existed: gram_block's loop over the pairs of groups and its two
scatter loops, a launch at a time, and vc_point's batch loop with its profile line.  tests/test_stats_plan_host.py holds the compiled header to this
file."""
import numpy as np

import _sweep_plan as SP

K_GRAM_MAX_COLS = 4096
OFF_C, OFF_Q, REC = 10 * 256, 10 * 256 + 64, 10 * 256 + 64 + 1                   # GramRec<4>::OFF_C, OFF_Q, N

# A deliberate error for test_stats_plan_host to plant, one at a time (None: the plans as they are):
#   "pairs_b_outer"     the pairs of groups with b as the outer loop
#   "one_launch_le_65"  the single launch up to 65 columns
#   "jb1_floor"         a batch's last base column rounded down: the straddling group left to the next batch alone
FAULT = None


def _ceil(a, b):
    return -(-a // b)


def rec_g(s, l):
    """GramRec<4>::g: record offset of G[s][l], s <= l, in upper-triangular 16 x 16 tiles, row-major."""
    gs, gl = s >> 4, l >> 4
    return (gs * 4 - gs * (gs - 1) // 2 + (gl - gs)) * 256 + (s & 15) * 16 + (l & 15)


# ---- gram_block -----------------------------------------------------------------------------------------------------------------
def gram_launch_groups(m):
    """The launches of gram_block over m listed columns, in order, one row each: (a0, na, b0, nb) -- positions [a0, a0 + na) of
    the call's list, then [b0, b0 + nb).  (The loops over the pairs a < b of 32-column groups, a outer, as index arrays.)"""
    if m <= (65 if FAULT == "one_launch_le_65" else 64):
        return np.array([[0, m, m, 0]], dtype=np.int64)
    ng = (m + 31) // 32
    a, b = np.triu_indices(ng, 1)                                # for a in range(ng): for b in range(a + 1, ng)
    if FAULT == "pairs_b_outer":
        b, a = np.tril_indices(ng, -1)                           # for b in range(ng): for a in range(b)
    a0, b0 = 32 * a, 32 * b
    a1, b1 = np.minimum(a0 + 32, m), np.minimum(b0 + 32, m)
    return np.stack([a0, a1 - a0, b0, b1 - b0], axis=1).astype(np.int64)


def gram_launches(m):
    """... and for each launch the positions of the call's list it holds, by position inside the launch."""
    return [list(range(a0, a0 + na)) + list(range(b0, b0 + nb)) for a0, na, b0, nb in gram_launch_groups(m).tolist()]


REC_G = np.array([[rec_g(min(i, j), max(i, j)) for j in range(64)] for i in range(64)])   # rec_g(min, max) by position pair


def gram_scatter(m, records):
    """gram_block's two scatter loops: records[t] is the record launch t brought back; -> (out_G (m x m), out_c, out_q),
    NaN where nothing was written.  Each loop over the positions of ONE launch is written as one numpy assignment (its
    columns are distinct, so the order inside it cannot show); the launches follow each other as the loops did."""
    out_G, out_c, out_q = np.full((m, m), np.nan), np.full(m, np.nan), np.nan
    if m <= 64:
        rec = records[0]
        out_G[:, :] = rec[REC_G[:m, :m]]                         # out_G[i * m + j] = rec[R::g(min(i, j), max(i, j))]
        out_c[:] = rec[OFF_C:OFF_C + m]                          # out_c[i] = rec[R::OFF_C + i]
        out_q = rec[OFF_Q]
        return out_G, out_c, out_q
    ng, t = (m + 31) // 32, 0
    for a in range(ng):
        for b in range(a + 1, ng):
            a0, b0 = 32 * a, 32 * b
            a1, b1 = min(a0 + 32, m), min(b0 + 32, m)
            na, nb = a1 - a0, b1 - b0
            rec = records[t]
            t += 1
            col_of = np.array([a0 + pos if pos < na else b0 + (pos - na) for pos in range(na + nb)])
            out_G[np.ix_(col_of, col_of)] = rec[REC_G[:na + nb, :na + nb]]     # out_G[i * m + col_of(pj)] = rec[R::g(min(pi, pj), max(pi, pj))]
            out_c[col_of] = rec[OFF_C:OFF_C + na + nb]                         # out_c[i] = rec[R::OFF_C + pi]
            out_q = rec[OFF_Q]
    return out_G, out_c, out_q


# ---- vc_point -------------------------------------------------------------------------------------------------------------------
def vc_point_plan(p, degree, n, dtype, cus, loo):
    """vc_point's loop over the k_col_dots batches of expanded columns (degree >= 1): per batch (b0, b1, jb0, jb1, chunks, table,
    doubles asked of need_partials); then the launches and bytes of its profile line."""
    Q1 = degree + 1
    batches, launches = [], 1
    if degree > 0:
        for b0 in range(0, p, SP.K_COL_BATCH):
            b1 = min(b0 + SP.K_COL_BATCH, p)
            chunks = SP.col_dots_plan(b1 - b0, n, dtype, cus, 1)[1]
            jb0, jb1 = b0 // Q1, (b1 // Q1 if FAULT == "jb1_floor" else (b1 + Q1 - 1) // Q1)
            table = (jb1 - jb0) * Q1 * chunks
            batches.append((b0, b1, jb0, jb1, chunks, table, table * (2 if loo else 1)))
            launches += 1
    return batches, launches, float(n) * float(SP.esz(dtype)) * (float(p) + 2.0)
