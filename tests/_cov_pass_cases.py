"""Constructed cases for the cache-served full pass that the host drives (gc_pass_device and the windowed walk of gc_full_pass,
csrc/grad_cache.hpp; k_cov_scan, k_cov_block, k_cov_gupdate_chk, k_cov_restore, k_cov_pack, csrc/gram_kernels.hpp), and the
oracle's account of each.  numpy and the CPU oracle only: tests/test_cov_pass_cases_host.py checks on the CPU that every case
is what it declares, tests/test_gpu_cov_pass_edges.py runs them on the device.

Random data cannot place a broken certificate, so the Gram matrix is built entry by entry: X = s I (n = p) plus a few
couplings; a coupling (j -> k, c) adds c to row j of column k, which makes G_jk = s c and G_kk = s^2 + c^2 and leaves every
other pair orthogonal (no row carries two couplings).  The start is chosen through the gradient: pick g0 = X'W r0 freely, solve
for r0 (exactly: the couplings form chains), set y = r0 + X beta0.  With lambda = 1/2, s = 4 and c in {3, 4, 8} every number
of a least-squares case is a small dyadic rational and every sum is exact in fp64 and in fp32.

The pieces (T_k = lambda n omega_k is the threshold |g_k| is held against, u_k = T_k / a_k):
  filler    a support coordinate with beta0 = 4 u, g0 = -T/4: moves by h = -1.25 u in pass 1, by exactly 0 from then on
  stuck     a support coordinate with g0 = +T: unsettled, h = 0 exactly
  target    beta0 = 0, g0 = -T/4, coupled to a filler j with c = 2 s: j's move takes g to +2.25 T.  Its certificate, read at the
            scan, breaks at its turn if and only if j is visited before it
  entering  beta0 = 0, |g0| = 1.5 T
  the rest  beta0 = 0, g0 = +-T/4 (never zero: an exact zero sends the pass to the walk; one case is there for that exit)

Positions and coordinates are 0-based here; the visit lists go to the libraries 1-based."""
import functools
from dataclasses import dataclass, field

import numpy as np

S = 4.0
LAM = 0.5
LAM_SQRT = 2.0
THR_MARGIN = 1.0 - 1e-9          # kThrMargin, csrc/kernels.hpp
MAX_FORCED_ROUNDS = 4            # kMaxForcedRounds, csrc/cov_solve_types.hpp
GC_BUSY = 64                     # kGcBusy, csrc/cdhip.hip
GC_COV_WINDOW = 2048             # kGcCovWindow, csrc/cdhip.hip
COORD, B16, B32, B64 = ("coord", 0), ("block", 16), ("block", 32), ("block", 64)


def width(mode):
    """launch_cov_blocks' block width for a sweep mode"""
    return mode[1] if mode[0] == "block" and mode[1] >= 16 else 16


@dataclass(frozen=True, eq=False)
class Case:
    id: str
    group: str
    loss: str                     # "ls", "sqrt", "wls"
    p: int
    mode: tuple
    lam: float
    couplings: tuple              # (j, k, c): row j of column k carries c
    beta0: np.ndarray = field(repr=False)
    r0: np.ndarray = field(repr=False)
    lists: tuple = field(repr=False)      # one 0-based visit list per pass
    omega: np.ndarray = field(default=None, repr=False)
    w: np.ndarray = field(default=None, repr=False)
    # declared about pass 1
    U: int = 0                    # unsettled positions at the scan
    breaks: tuple = ()            # positions whose certificate breaks at their turn
    forced_rounds: int = 0
    rollbacks: int = 0
    device: bool = True           # the pass completes on the device
    served: bool = True           # the pass is served from the cache at all (False: it backs off to the plain path)
    zero_g: tuple = ()            # coordinates with g0 == 0 exactly
    still: bool = False           # every h of pass 2 is exactly zero
    f32: bool = False             # also run in fp32 storage
    walk_break: bool = False      # the walk itself must re-run a window in pass 1

    @property
    def nnz0(self):
        return int(np.count_nonzero(self.beta0))


# ---- least squares and weighted least squares -----------------------------------------------------------------------------------
def _ls(id, group, p, mode, lists, fillers=(), pairs=(), *, stuck=(), enter=(), zero=(), omega=None, w=None, g0_over=None,
        beta_over=None, **declared):
    """pairs: (j, k, c).  g0_over / beta_over: {coordinate: multiple of T_k / of u_k}."""
    lists = tuple(np.ascontiguousarray(l, dtype=np.int64) for l in lists)
    om = np.ones(p) if omega is None else np.asarray(omega, dtype=np.float64)
    wt = np.ones(p) if w is None else np.asarray(w, dtype=np.float64)
    rows = [j for j, _, _ in pairs]
    assert len(set(rows)) == len(rows), "one coupling per row, or two targets stop being orthogonal"
    a = S * S * wt
    for j, k, c in pairs:
        a[k] += wt[j] * c * c
    T = LAM * p * om
    u = T / a
    g0 = 0.25 * T * np.where(np.arange(p) % 2 == 0, 1.0, -1.0)
    beta0 = np.zeros(p)
    for _, k, _ in pairs:
        g0[k] = -0.25 * T[k]
    for j in fillers:
        beta0[j], g0[j] = 4.0 * u[j], -0.25 * T[j]
    for j in stuck:
        beta0[j], g0[j] = 4.0 * u[j], T[j]
    for k in enter:
        g0[k] = 1.5 * T[k] * (1.0 if k % 2 == 0 else -1.0)
    for k in zero:
        g0[k] = 0.0
    for k, v in (g0_over or {}).items():
        g0[k] = v * T[k]
    for k, v in (beta_over or {}).items():
        beta0[k] = v * u[k]
    # X'W r = g0, column k: s w_k r_k + sum over its couplings of c w_j r_j; the couplings form chains, so a few sweeps settle it
    r = g0 / (S * wt)
    for _ in range(len(pairs) + 1):
        nxt = g0.copy()
        for j, k, c in pairs:
            nxt[k] -= c * wt[j] * r[j]
        r = nxt / (S * wt)
    loss = "wls" if w is not None else "ls"
    return Case(id=id, group=group, loss=loss, p=p, mode=mode, lam=LAM, couplings=tuple(pairs), beta0=beta0, r0=r, lists=lists,
                omega=None if omega is None else om, w=None if w is None else wt, zero_g=tuple(zero), **declared)


def _ident(p, passes=3):
    return tuple(np.arange(p) for _ in range(passes))


def _group_a():
    out = []
    for mode in (COORD, B16, B32, B64):
        B = width(mode)
        p = 528 if B == 64 else 272                      # nnz 4 <= p at U = 2B + 1
        for U in (1, B - 1, B, B + 1, 2 * B, 2 * B + 1):
            fillers = [1 + 4 * i for i in range(U)]
            out.append(_ls(f"a-{mode[0]}{mode[1]}-U{U}", "a", p, mode, _ident(p, 2), fillers, U=U, still=True, f32=True))
    return out


def _placed(id, B, t, v, *, stuck=(), extra=(), **declared):
    """U = 2B + 1 fillers (three blocks of width B) at positions P_i = 5 + 8 i (B = 16) or 3 + 4 i; coordinate t is coupled to
    visit v's coordinate.  Its certificate breaks iff P_v < t."""
    mode = {16: COORD, 32: B32, 64: B64}[B]
    p = 528 if B == 64 else 272
    P = [(5 + 8 * i) if B == 16 else (3 + 4 * i) for i in range(2 * B + 1)]
    pairs = [(P[v], t, 2 * S)] + [(P[vv], tt, 2 * S) for vv, tt in extra]
    fillers = [x for x in P if x not in stuck]
    brk = tuple(sorted(tt for j, tt, _ in pairs if j < tt))
    return _ls(id, "b", p, mode, _ident(p), fillers, pairs, stuck=stuck, U=2 * B + 1, breaks=brk,
               forced_rounds=1 if brk else 0, **declared), P


def _group_b():
    out = []
    P = [5 + 8 * i for i in range(33)]
    for name, t, before, after in (("inside", P[5] + 1, 5, 6),                 # right after the mover, inside block 0
                                   ("between", P[15] + 1, 15, 16),             # behind block 0's last visit, before block 1's first
                                   ("last-1", P[31] - 1, 30, 31),              # t = upos[j0 + nb - 1] - 1 of block 1
                                   ("prev+1", P[31] + 1, 31, 32)):             # t = upos[j0 - 1] + 1 of block 2
        out.append(_placed(f"b-{name}-break", 16, t, before)[0])
        out.append(_placed(f"b-{name}-mirror", 16, t, after)[0])
    out.append(_placed("b-prev+1-far-mover-break", 16, P[15] + 1, 0)[0])    # owned by block 1, moved in block 0
    out.append(_placed("b-tail-break", 16, P[32] + 1, 32)[0])              # behind the last visit of the pass
    out.append(_placed("b-tail-end-break", 16, 271, 20)[0])                # t = m - 1
    out.append(_placed("b-before-first-visit", 16, 2, 10)[0])              # its mover comes later, wherever: never flagged
    # block 0's last visit is unsettled and does not move: p_last comes from a position the compacted mover list does not hold
    out.append(_placed("b-stuck-last-visit", 16, P[15] - 1, 14, stuck=(P[15],), extra=((13, P[15] + 1),))[0])
    for B in (32, 64):                                   # the same block edges at NG = 2 and 4
        Pb = [3 + 4 * i for i in range(2 * B + 1)]
        out.append(_placed(f"b-between-break-B{B}", B, Pb[B - 1] + 1, B - 1)[0])
        out.append(_placed(f"b-between-mirror-B{B}", B, Pb[B - 1] + 1, B)[0])
        out.append(_placed(f"b-tail-end-break-B{B}", B, (528 if B == 64 else 272) - 1, B + 3)[0])
    return out


def _group_c():
    out = []
    for p in (1023, 1024, 1025, 2049):
        uns = [q for q in (3, 500, 1022, 1023, 1024, 1025, 2047, 2048) if q < p]
        j, t = (1023, 1500) if p == 2049 else (500, 700)           # p = 2049: the mover below 1024, its target above
        out.append(_ls(f"c-scan-p{p}", "c", p, COORD, _ident(p), uns, [(j, t, 2 * S)], U=len(uns), breaks=(t,), forced_rounds=1,
                       f32=True))
    # a list of 1024 (one turn of the scan's loop) that visits all twelve fillers, then the full list twice: the scan's second turn
    # then appends to a compaction whose slots an earlier pass has filled
    p = 2049
    uns = [3, 100, 200, 300, 400, 500, 1022, 1023, 1024, 1025, 2047, 2048]
    short = np.array([q for q in range(1024) if q not in (10, 11, 12, 13)] + [1024, 1025, 2047, 2048])
    out.append(_ls("c-scan-p2049-after-short-list", "c", p, COORD, (short, np.arange(p), np.arange(p)), uns, [(500, 700, 2 * S)], U=12,
                   breaks=(int(np.flatnonzero(short == 700)[0]),), forced_rounds=1, f32=True))
    p = 272
    third = np.arange(0, p, 3)
    # every third coordinate, then everything: 31 is not listed in pass 1 and must be seen moved in pass 2; 61 breaks in pass 1
    out.append(_ls("c-partial-list", "c", p, COORD, (third, np.arange(p), np.arange(p)), [30, 60, 150], [(30, 31, 2 * S), (60, 63, 2 * S)],
                   U=3, breaks=(21,), forced_rounds=1, f32=True))
    perm = np.random.default_rng(7).permutation(p)
    sup = [int(perm[q]) for q in (9, 100, 151, 260)]
    out.append(_ls("c-permuted-list", "c", p, COORD, (perm, perm, perm), sup,
                   [(int(perm[100]), int(perm[101]), 2 * S), (int(perm[151]), int(perm[150]), 2 * S)],
                   U=4, breaks=(101,), forced_rounds=1, f32=True))
    A, Brev = np.arange(p), np.arange(p)[::-1].copy()
    out.append(_ls("c-lists-A-B-A", "c", p, COORD, (A, Brev, A), [10, 100, 200], [(100, 101, 2 * S)], U=3, breaks=(101,), forced_rounds=1,
                   f32=True))
    return out


def _group_d():
    out = []
    for p in (255, 256, 257):
        out.append(_ls(f"d-p{p}-broken-last", "d", p, COORD, _ident(p), [10, 50, 90], [(90, p - 1, 2 * S)], U=3, breaks=(p - 1,),
                       forced_rounds=1))
        rev = np.arange(p)[::-1].copy()
        out.append(_ls(f"d-p{p}-mover-last", "d", p, COORD, (rev, rev, rev), [10, 50, p - 1], [(p - 1, p - 2, 2 * S)], U=3, breaks=(1,),
                       forced_rounds=1))
    return out


def _sqrt(id, p, movers, k, order, **declared):
    """Sqrt-lasso, X = s I, no couplings: coordinate k has |g_k| = 0.9 lambda ||r0|| and only ||r|| changes.  movers: (j, f): a
    support coordinate whose visit leaves ||r|| = f ||r0|| (the fractions are of r0 and fall from mover to mover).
    A visit of j leaves r'r = gamma (r'r - r_j^2) with gamma = s^2 / (s^2 - lambda^2), whatever beta_j was."""
    lam, gam = LAM_SQRT, S * S / (S * S - LAM_SQRT * LAM_SQRT)
    rest = [q for q in range(p) if q != k and q not in [j for j, _ in movers]]
    R0 = float(len(rest))                            # the rest: r = +-1
    # N = r0'r0 = R0 + t^2 + sum J_j^2 with t^2 = (0.9 lambda)^2 N / s^2 and J_1^2 = N (1 - f1^2 / gamma), J_2^2 = N (f1^2 - f2^2 / gamma) ...
    shares, prev = [], 1.0
    for _, f in movers:
        shares.append(prev - f * f / gam)
        prev = f * f
    tshare = (0.9 * lam / S) ** 2
    N = R0 / (1.0 - tshare - sum(shares))
    assert N > 0 and all(sh > 0 for sh in shares)
    r = np.where(np.arange(p) % 2 == 0, 1.0, -1.0)
    r[k] = np.sqrt(tshare * N)
    beta0 = np.zeros(p)
    for (j, _), sh in zip(movers, shares):
        r[j] = np.sqrt(sh * N)
        beta0[j] = 1.0
    lst = np.ascontiguousarray(order, dtype=np.int64)
    return Case(id=id, group="e", loss="sqrt", p=p, mode=COORD, lam=lam, couplings=(), beta0=beta0, r0=r, lists=(lst, lst, lst),
                U=len(movers), **declared)


def _group_e():
    p = 64
    om_small, om_large = np.ones(p), np.ones(p)
    om_small[21], om_large[21] = 0.5, 4.0
    out = [
        # c = 3: g_21 goes from -T0/8 to +0.8125 T0 -- settled at omega = 1, broken only because omega_21 = 1/2
        _ls("e-omega-small-break", "e", p, COORD, _ident(p), [5, 20, 40], [(20, 21, 3.0)], omega=om_small, g0_over={21: -0.25}, U=3,
            breaks=(21,), forced_rounds=1),
        # c = 8: g_21 goes to +2.25 T0 -- broken at omega = 1, settled only because omega_21 = 4
        _ls("e-omega-large-holds", "e", p, COORD, _ident(p), [5, 20, 40], [(20, 21, 2 * S)], omega=om_large, g0_over={21: -0.0625}, U=3),
    ]
    w = np.array([1.0, 2.0, 4.0])[np.arange(p) % 3]
    out.append(_ls("e-wls-break", "e", p, COORD, _ident(p), [5, 20, 40], [(20, 21, 2 * S)], w=w, U=3, breaks=(21,), forced_rounds=1))
    out.append(_ls("e-wls-mirror", "e", p, COORD, _ident(p), [5, 22, 40], [(22, 21, 2 * S)], w=w, U=3))
    ident = np.arange(p)
    out.append(_sqrt("e-sqrt-q-break", p, [(10, 0.8)], 20, ident, breaks=(20,), forced_rounds=1))
    out.append(_sqrt("e-sqrt-q-mirror", p, [(20, 0.8)], 10, ident))
    out.append(_sqrt("e-sqrt-q-second-mover-only", p, [(10, 0.97), (30, 0.8)], 20, ident))       # must not be flagged
    out.append(_sqrt("e-sqrt-q-first-mover-already", p, [(10, 0.8), (30, 0.7)], 20, ident, breaks=(20,), forced_rounds=1))
    return out


def _chain(L, p, j, links, fillers=(), **declared):
    """j moves by -64 u and takes g_k1 to 64.25 T; each link's own move (c = s: a = 2 s^2, G = s^2) takes the next one's
    gradient to about half of that with the other sign: 64.25, -31.875, 15.6875, -7.59, 3.55 (times T)."""
    pairs = [(j, links[0], S)] + [(links[i], links[i + 1], S) for i in range(L - 1)]
    g0 = {j: -63.0}
    g0.update({k: 0.25 if i % 2 == 0 else -0.25 for i, k in enumerate(links)})
    return _ls(f"f-chain-L{L}", "f", p, COORD, _ident(p), list(fillers), pairs, g0_over=g0, beta_over={j: 70.0},
               U=1 + len(fillers), breaks=tuple(links), **declared)


def _group_f():
    out = [_chain(L, 64, 2, [10, 20, 30, 40][:L], forced_rounds=L) for L in (1, 2, 3, 4)]
    # L = 5: the fifth round is not granted; the pass is undone once and the walk finishes it.  64 fillers between one link and the
    # next: the walk cuts its windows at 64 unsettled visits, so every link is in the window after its mover's and the walk
    # itself re-runs nothing
    links = [65 * i for i in range(1, 6)]
    fillers = [q for q in range(1, 326) if q % 65 != 0]
    out.append(_chain(5, 1312, 0, links, fillers, forced_rounds=MAX_FORCED_ROUNDS, rollbacks=1, device=False))
    return out


def _group_g():
    # 32 fillers: their Gram columns are one full batch, so preparing the pass fetches none of the entering coordinates' columns
    p, sup = 400, [1 + 4 * i for i in range(32)]
    out = [_ls("g-enter-64", "g", p, COORD, _ident(p), sup, enter=[130 + 4 * i for i in range(GC_BUSY)], U=32 + GC_BUSY),
           _ls("g-enter-65", "g", p, COORD, _ident(p), sup, enter=[130 + 4 * i for i in range(GC_BUSY + 1)], U=32 + GC_BUSY + 1,
               device=False, served=False),
           # nothing in the support: the handle holds no Gram column at all yet, and gc_pass_device leaves such a pass to the walk,
           # which fetches the 64 columns and serves it
           _ls("g-enter-64-cold", "g", 272, COORD, _ident(272), enter=[2 + 4 * i for i in range(GC_BUSY)], U=GC_BUSY, device=False),
           # entering coordinates before and behind the exact zero: the order of the support depends on the settled visits' bookkeeping
           _ls("g-exact-zero", "g", 64, COORD, _ident(64), [5, 40], enter=[15, 50], zero=[30], U=4, device=False)]
    return out


def _group_w():
    """The walk's own cuts (these run on the device pass too, where they are one more break each)."""
    p = 2049
    # the first window is [0, 2048): position 2047 is its last, skipped, and broken by the visit at 2046; it then opens the second
    # window.  (A list of 2049 positions leaves the second window one position, so the break cannot lie strictly inside it.)
    out = [_ls("w-window-2048", "w", p, COORD, _ident(p), [0, 2045, 2046, 2048], [(2046, 2047, 2 * S)], U=4, breaks=(2047,), forced_rounds=1,
               walk_break=True)]
    # 65 unsettled visits at B = 16: the first window takes 64 of them, the break lies behind the 65th
    p = 272
    P = [1 + 4 * i for i in range(65)]
    out.append(_ls("w-maxlen-64", "w", p, COORD, _ident(p), P, [(P[64], P[64] + 2, 2 * S)], U=65, breaks=(P[64] + 2,), forced_rounds=1,
                   walk_break=True))
    return out


A, Bg, Cg, D, E, F, G, W = _group_a(), _group_b(), _group_c(), _group_d(), _group_e(), _group_f(), _group_g(), _group_w()
ALL = A + Bg + Cg + D + E + F + G + W
BY_ID = {c.id: c for c in ALL}
assert len(BY_ID) == len(ALL)
F32 = [c for c in ALL if c.f32]
SOLVES = [c for c in ALL if c.loss in ("ls", "sqrt") and c.nnz0 <= 100]


# ---- the data of a case ------------------------------------------------------------------------------------------------------
def design(case):
    X = np.zeros((case.p, case.p), order="F")
    X[np.arange(case.p), np.arange(case.p)] = S
    for j, k, c in case.couplings:
        X[j, k] += c
    return X


@functools.lru_cache(maxsize=2)
def data(case):
    """-> (X, y), read-only and shared.  n = p."""
    X = design(case)
    y = case.r0 + X @ case.beta0
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def perturbed(case, copy):
    """X and y with independent relative 1e-13 noise (copy = 1, 2, 3)"""
    X, y = data(case)
    rng = np.random.default_rng(10 ** 6 * copy + case.p)
    return np.asfortranarray(X * (1.0 + 1e-13 * rng.standard_normal(X.shape))), y * (1.0 + 1e-13 * rng.standard_normal(y.shape))


def make(mod, case, X, y):
    """(loss, penalty, iterate) of the case in `mod`: the oracle, or the device library"""
    if case.loss == "wls":
        f = mod.CDWeightedLSLoss(y, X, case.w)
    else:
        f = (mod.CDSqrtLassoLoss if case.loss == "sqrt" else mod.CDLeastSquaresLoss)(y, X)
    return f, mod.ProxL1(case.lam, case.omega), mod.SparseIterate(case.p, case.beta0)


def gc_cert_abs(case, y, roundings=64):
    """gc_cert_abs (csrc/grad_cache.hpp) for fp32 storage, restated: 2^-24 sqrt(y'Wy / n) (64 sqrt(U + 1) + 512), U the number of
    times the residual was rewritten since it was rebuilt (64 is far more than three passes do)"""
    yy = float(np.sum((case.w if case.w is not None else 1.0) * y * y))
    return 2.0 ** -24 * np.sqrt(yy / case.p) * (64.0 * np.sqrt(roundings + 1.0) + 512.0)


# ---- the oracle's account ----------------------------------------------------------------------------------------------------
def _unsettled(beta, g, thr, a):
    """cov_settled's rule, negated (csrc/gram_kernels.hpp)"""
    return (beta != 0.0) | ~(a > 0.0) | (np.abs(g) > thr * THR_MARGIN)


def _thr(case, r):
    om = 1.0 if case.omega is None else case.omega
    w = 1.0 if case.w is None else case.w
    return case.lam * om * (np.sqrt(float(np.sum(w * r * r))) if case.loss == "sqrt" else float(case.p))


def _thr_k(case, r, k):
    t = _thr(case, r)
    return float(t[k]) if np.ndim(t) else float(t)


def trace(case, X=None, y=None):
    """The oracle's passes over the case's lists, one visit at a time, with X_k'W r and the threshold at the scan and at each
    coordinate's turn.  -> {"passes": [per pass], "r": residual at the end}.  Per pass: lst, g_scan, thr_scan, beta_scan (all p),
    g_turn, thr_turn, h (per position), uns_scan, uns_turn (per position), V (positions), rounds, visited (positions the
    device's rounds end up visiting), beta, support, maxH."""
    import oracle as O
    if X is None:
        X, y = data(case)
    f, g, x = make(O, case, X, y)
    O.initialize_(f, x)
    w = np.ones(case.p) if case.w is None else case.w
    a = np.einsum("ij,ij->j", X, X * w[:, None]) if case.w is not None else np.einsum("ij,ij->j", X, X)
    out = []
    for lst in case.lists:
        m = len(lst)
        beta_scan, r_scan = x.dense(), np.array(f.r)
        g_scan, thr_scan = X.T @ (w * r_scan), _thr(case, r_scan) * np.ones(case.p)
        g_turn, thr_turn, h = np.zeros(m), np.zeros(m), np.zeros(m)
        for q, k in enumerate(lst):
            r = f.r
            g_turn[q] = float(X[:, k] @ (w * r))
            thr_turn[q] = _thr_k(case, r, k)
            h[q] = O.descendCoordinate_(f, g, x, int(k) + 1)
        x.dropzeros()
        uns_scan = _unsettled(beta_scan[lst], g_scan[lst], thr_scan[lst], a[lst])
        uns_turn = _unsettled(beta_scan[lst], g_turn, thr_turn, a[lst])
        rounds, visited = _rounds(case, X, y, w, a, beta_scan, lst, uns_scan)
        out.append({"lst": lst, "g_scan": g_scan, "thr_scan": thr_scan, "beta_scan": beta_scan, "g_turn": g_turn, "thr_turn": thr_turn,
                    "h": h, "uns_scan": uns_scan, "uns_turn": uns_turn, "V": np.flatnonzero(uns_scan | uns_turn), "rounds": rounds,
                    "visited": visited, "beta": x.dense(), "support": np.asarray(x.nzval2ind).tolist(),
                    "maxH": float(np.max(np.abs(h))) if m else 0.0})
    return {"passes": out, "r": np.array(f.r)}


def _rounds(case, X, y, w, a, beta_scan, lst, uns_scan):
    """gc_pass_device's rounds, played with the oracle's visits: only the listed positions are visited, every skipped one is held
    against X_k'W r at its turn, the broken ones join the list and the pass starts over.  -> (rounds beyond the first, the
    positions visited in the last).  No cap: the chain length."""
    import oracle as O
    visit = uns_scan.copy()
    for rounds in range(len(lst) + 1):
        f, g, _ = make(O, case, X, y)
        x = O.SparseIterate(case.p, beta_scan)
        O.initialize_(f, x)
        broken = np.zeros(len(lst), dtype=bool)
        for q, k in enumerate(lst):
            if visit[q]:
                O.descendCoordinate_(f, g, x, int(k) + 1)
            else:
                r = f.r
                gk = float(X[:, k] @ (w * r))
                thr = _thr_k(case, r, k)
                broken[q] = bool(_unsettled(beta_scan[k:k + 1], np.array([gk]), np.array([thr]), a[k:k + 1])[0])
        if not broken.any():
            return rounds, np.flatnonzero(visit)
        visit |= broken
    raise AssertionError(case.id)


@functools.lru_cache(maxsize=None)
def oracle_of(case):
    """the trace of the case as given: computed once, shared, not to be written to"""
    return trace(case)


def discrete(tr):
    """what must not hang on the last bits: per pass, who is unsettled at the scan and at its turn, the rounds, the support"""
    return [(tuple(np.flatnonzero(ps["uns_scan"])), tuple(np.flatnonzero(ps["uns_turn"])), ps["rounds"], tuple(ps["visited"]),
             tuple(ps["support"])) for ps in tr["passes"]]


def solve_oracle(case, X=None, y=None):
    """the warm-started solve from beta0 -> (beta, passes, visits, converged, support)"""
    import oracle as O
    if X is None:
        X, y = data(case)
    f, g, x = make(O, case, X, y)
    st = O.coordinateDescent_(x, f, g, O.CDOptions(maxIter=500, optTol=1e-10, randomize=False, warmStart=True))
    return x.dense(), st["passes"], st["visits"], st["converged"], np.asarray(x.nzval2ind).tolist()
