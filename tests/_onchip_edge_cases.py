"""The cases of tests/test_gpu_onchip_edges.py: k_solve_small (csrc/small_solve.hpp) at the sizes where it changes what it does
-- the three unroll widths (p <= 256, <= 512, larger), the visit list's chunks of 64, the two shuffle constructions of
wave_build_list (L <= 64 in registers, longer lists by parallel_fisher_yates), wave_dropzeros over several chunks, the Gram
column cache running full (`_small_plan.ncache(p)` columns), warm starts with more than 64 non-zeros -- and the ONE helper
that runs a case on the device and holds it to the oracle.

Kept apart from the GPU module so that tests/test_onchip_edge_cases_host.py (no GPU) can run the oracle on every case here
and on perturbed copies: the kernel visits in covariance form, the oracle on the residual, so equal pass counts and support
ORDER are only a fair demand of a case whose own outcome does not hang on the last bits."""
import ctypes as C
import functools
from dataclasses import dataclass, replace

import numpy as np

import oracle as O
import _small_plan as SP

BETA_TOL = 1e-10             # |beta - oracle|_inf <= BETA_TOL max(1, |oracle|_inf) at every lambda
RESID_TOL = 1e-9
F32_TOL = 3e-4               # fp32 storage against the fp64 oracle on the fp32-rounded inputs

# fractions of the problem's own lambda_max (max_k |X_k'y| / n, sqrt-lasso: / ||y||; over omega_k where weighted).  Chosen on
# the oracle alone so that check_design holds: the support is below 64 after the first lambda and beyond 64 -- and beyond the
# column cache -- after the last (45 -> 86 -> 132 at p = 1024, ls; 31 -> 103 -> 191, sqrt)
FRACTIONS = {"ls": (0.3, 0.1, 0.03), "sqrt": (0.5, 0.3, 0.17), "wls": (0.3, 0.1, 0.03)}
MATRIX_P = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024)


@dataclass(frozen=True)
class Case:
    id: str
    loss: str                     # "ls", "sqrt", "wls"
    p: int
    n: int
    seed: int
    randomize: bool
    s: int                        # true support
    must: tuple = ()              # 1-based coordinates the true support includes
    fractions: tuple = None       # of lambda_max; None: `lams` are absolute
    lams: tuple = ()
    x0: str = ""                  # "", "small150", "small70", "small200", "near130"
    weights: bool = False         # observation weights (one exact zero) and penalty weights (one exact zero)
    warm: bool = True
    max_iter: int = 20000
    entry: str = "cd"             # "cd": coordinateDescent! (g = X'y - G beta); "solve": cdh_solve (g = X'r)
    f32: bool = False
    opt_tol: float = 1e-12
    coef: float = 0.0             # > 0: the true coefficients are +-(coef .. 2 coef) instead of standard normal


def _n_of(p):
    return max(300, min(1500, 2 * p))


def _matrix():
    out = []
    for i, p in enumerate(MATRIX_P):
        must = (63, 64, 65, p) if p >= 65 else ()
        for loss in ("ls", "sqrt"):
            for rand in (False, True):
                out.append(Case(id=f"{loss}-p{p}-{'shuffled' if rand else 'ordered'}", loss=loss, p=p, n=_n_of(p), seed=9100 + i,
                                randomize=rand, s=min(p // 2, 120), must=must, fractions=FRACTIONS[loss]))
    return out


MATRIX = _matrix()
WEIGHTED = [Case(id=f"wls-p{p}-shuffled", loss="wls", p=p, n=_n_of(p), seed=9200 + p, randomize=True, s=min(p // 2, 120),
                 must=(63, 64, 65, p), fractions=FRACTIONS["wls"], weights=True) for p in (65, 513, 1024)]
COLD = [Case(id="ls-p1024-cold-shuffled", loss="ls", p=1024, n=1500, seed=9301, randomize=True, s=120, must=(63, 64, 65, 1024),
             fractions=(0.03,), warm=False)]
CUT = [Case(id=f"ls-p{p}-maxiter3-{'shuffled' if rand else 'ordered'}", loss="ls", p=p, n=_n_of(p), seed=9400 + p, randomize=rand,
            s=120, must=(63, 64, 65, p), fractions=(0.03,), max_iter=3) for p in (513, 1024) for rand in (False, True)]
DROPZEROS = [Case(id=f"ls-p300-{x0}-{'shuffled' if rand else 'ordered'}", loss="ls", p=300, n=600, seed=9500, randomize=rand, s=s,
                  lams=(lam,), x0=x0, coef=1.0)
             for x0, s, lam in (("small150", 6, 0.2), ("small70", 6, 0.2), ("small200", 80, 0.2)) for rand in (False, True)]
DROPZEROS = [replace(c, must=(295, 296, 297, 298, 299, 300)) if c.x0 == "small70" else c for c in DROPZEROS]
LONG_WARM = [Case(id=f"{loss}-p513-near130-{entry}", loss=loss, p=513, n=1026, seed=9600, randomize=True, s=130, must=(63, 64, 65, 513),
                  fractions=(FRACTIONS[loss][1],), x0="near130", entry=entry) for loss in ("ls", "sqrt") for entry in ("cd", "solve")]
F32 = [Case(id=f"ls-p{p}-f32-ordered", loss="ls", p=p, n=_n_of(p), seed=9700 + p, randomize=False, s=120, must=(63, 64, 65, p),
            fractions=FRACTIONS["ls"], f32=True, opt_tol=1e-6) for p in (513, 1024)]
OFF_CHIP = [c for c in MATRIX if c.p in (513, 1024)]
EXACT = MATRIX + WEIGHTED + COLD + CUT + DROPZEROS + LONG_WARM          # held to the oracle's discrete outcomes
ALL = EXACT + F32
BY_ID = {c.id: c for c in ALL}
assert len(BY_ID) == len(ALL)


@functools.lru_cache(maxsize=4)
def data(case):
    """-> dict(X, Y, w, omega, x0, lams): everything a run of the case reads.  Read-only: shared between tests."""
    rng = np.random.default_rng(case.seed)
    n, p = case.n, case.p
    X = np.asfortranarray(rng.standard_normal((n, p)))
    must = [k - 1 for k in dict.fromkeys(case.must)]
    rest = rng.permutation([k for k in range(p) if k not in must])
    sup = np.array(sorted(must + rest[: case.s - len(must)].tolist()), dtype=np.int64)
    beta = np.zeros(p)
    if case.coef > 0:
        beta[sup] = case.coef * rng.uniform(1.0, 2.0, size=sup.size) * rng.choice([-1.0, 1.0], size=sup.size)
    else:
        beta[sup] = rng.standard_normal(sup.size)
        beta[must] = np.sign(beta[must]) * (1.0 + np.abs(beta[must]))      # (the coordinates a case places are in its supports)
    Y = X @ beta + rng.standard_normal(n)
    w = omega = None
    if case.weights:
        w = rng.random(n) + 0.5
        w[n // 3] = 0.0
        omega = rng.uniform(0.5, 2.0, size=p)
        omega[p // 2] = 0.0
    if case.f32:
        X = np.asfortranarray(X.astype(np.float32))
        Y = Y.astype(np.float32)
    others = np.array([k for k in range(p) if beta[k] == 0.0])
    x0 = None
    if case.x0.startswith("small"):
        m = int(case.x0[5:])
        x0 = np.zeros(p)
        # SparseIterate takes the non-zeros in index order.  small70: the true support is the six HIGHEST coordinates (`must`), so
        # it holds the last slots, 64 .. 69 -- the holes of the first dropzeros! lie in chunk 0, its fillers in chunk 1
        junk = np.arange(m - sup.size) if case.x0 == "small70" else rng.permutation(others)[: m - sup.size]
        idx = np.concatenate([sup, junk])
        assert np.unique(idx).size == m
        x0[idx] = 1e-3 * rng.uniform(1.0, 2.0, size=idx.size) * rng.choice([-1.0, 1.0], size=idx.size)
    elif case.x0 == "near130":
        x0 = beta * (1.0 + 0.01 * rng.standard_normal(p))
    lams = case.lams
    if case.fractions is not None:
        Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
        c = np.abs(Xd.T @ ((w * Yd) if w is not None else Yd))
        if omega is not None:
            c = np.where(omega > 0, c / np.where(omega > 0, omega, 1.0), 0.0)
        lmax = float(np.max(c)) / (float(np.linalg.norm(Yd)) if case.loss == "sqrt" else n)
        lams = tuple(fr * lmax for fr in case.fractions)
    for a in (X, Y, w, omega, x0):
        if a is not None:
            a.setflags(write=False)
    return {"X": X, "Y": Y, "w": w, "omega": omega, "x0": x0, "lams": lams}


def perturbed(case, copy):
    """X and y with independent relative 1e-13 noise (copy = 1, 2, 3); everything else as given."""
    d = dict(data(case))
    rng = np.random.default_rng(10 ** 6 * copy + case.seed)
    d["X"] = np.asfortranarray(d["X"].astype(np.float64) * (1.0 + 1e-13 * rng.standard_normal(d["X"].shape)))
    d["Y"] = d["Y"].astype(np.float64) * (1.0 + 1e-13 * rng.standard_normal(d["Y"].shape))
    return d


def _options(case, mod, opt_tol=None):
    return mod.CDOptions(maxIter=case.max_iter, optTol=case.opt_tol if opt_tol is None else opt_tol, randomize=case.randomize,
                         warmStart=case.warm, seed=17)


def _loss(mod, case, d):
    if case.loss == "wls":
        return mod.CDWeightedLSLoss(d["Y"], d["X"], d["w"])
    return (mod.CDSqrtLassoLoss if case.loss == "sqrt" else mod.CDLeastSquaresLoss)(d["Y"], d["X"])


def run_oracle(case, d=None, opt_tol=None):
    """-> {"solves": [per lambda: beta, passes, visits, converged, support], "r": the residual at the end}"""
    d = data(case) if d is None else d
    d = dict(d, X=np.asfortranarray(d["X"], dtype=np.float64), Y=np.asarray(d["Y"], dtype=np.float64))
    f, x = _loss(O, case, d), O.SparseIterate(case.p, d["x0"])
    out = []
    for lam in d["lams"]:
        st = O.coordinateDescent_(x, f, O.ProxL1(lam, d["omega"]), _options(case, O, opt_tol))
        out.append({"beta": x.dense(), "passes": st["passes"], "visits": st["visits"], "converged": st["converged"],
                    "support": x.nzval2ind.tolist()})
    return {"solves": out, "r": np.array(f.r)}


@functools.lru_cache(maxsize=None)
def oracle_of(case):
    """the oracle's run of the case as given (computed once, shared, not to be written to); the fp32 cases: at optTol 1e-10"""
    return run_oracle(case, opt_tol=1e-10 if case.f32 else None)


def discrete(run):
    return [(s["passes"], s["visits"], s["converged"], tuple(s["support"])) for s in run["solves"]]


def run_device(cd, case, onchip=True):
    """The case on the device, through the entry it names -> the same record as run_oracle, plus "stats" (onchip_stats() at the
    end).  onchip=False: the same calls on the streamed per-coordinate sweep."""
    d = data(case)
    f, x = _loss(cd, case, d), cd.SparseIterate(case.p, d["x0"])
    try:
        if not onchip:
            f.set_onchip_solve(False)
            f.set_sweep_mode("coord")
        out = []
        for lam in d["lams"]:
            g, o = cd.ProxL1(lam, d["omega"]), _options(case, cd)
            if case.entry == "cd":
                cd.coordinateDescent_(x, f, g, o)
                st = f.last_stats
            else:
                # cdh_solve: "assumes r is initialised" -- initialize! first, then the solve takes g = X'r from the device's r
                f._set_penalty(g)
                f._push(x, rebuild=True)
                oc, cst = o._c(), cd._lib.cdh_stats()
                cd._lib.check(f._L.cdh_solve(f._h, C.byref(oc), C.byref(cst)), f._h)
                f._pull(x)
                st = {"passes": cst.passes, "visits": cst.visits, "converged": bool(cst.converged)}
            out.append({"beta": x.dense(), "passes": st["passes"], "visits": st["visits"], "converged": bool(st["converged"]),
                        "support": np.asarray(x.nzval2ind).tolist()})
        return {"solves": out, "r": np.array(f.r), "stats": f.onchip_stats()}
    finally:
        f.close()


def n_solves(case):
    return len(data(case)["lams"]) * (1 if case.warm else 51)


def hold_to(got, want, case, exact=True):
    """beta within BETA_TOL max(1, |beta|_inf) at every lambda, the same passes, visits, converged and support order, the residual
    at the end within RESID_TOL; printed before asserted.  exact=False (fp32 storage): beta within F32_TOL, nothing discrete."""
    tol = BETA_TOL if exact else F32_TOL
    for i, (a, b) in enumerate(zip(got["solves"], want["solves"])):
        scale = max(1.0, float(np.max(np.abs(b["beta"]))))
        err = float(np.max(np.abs(a["beta"] - b["beta"])))
        print(f"{case.id} lambda[{i}]: |beta - oracle| = {err:.3e} (bar {tol * scale:.1e}) passes {a['passes']} / {b['passes']} "
              f"visits {a['visits']} / {b['visits']} converged {a['converged']} / {b['converged']} nnz {len(a['support'])} / {len(b['support'])}")
    rerr = float(np.max(np.abs(got["r"].astype(np.float64) - want["r"])))
    print(f"{case.id}: |r - oracle| = {rerr:.3e}")
    assert len(got["solves"]) == len(want["solves"])
    for i, (a, b) in enumerate(zip(got["solves"], want["solves"])):
        scale = max(1.0, float(np.max(np.abs(b["beta"]))))
        np.testing.assert_allclose(a["beta"], b["beta"], rtol=0, atol=tol * scale, err_msg=f"{case.id} lambda[{i}]")
        if exact:
            assert (a["passes"], a["visits"], a["converged"]) == (b["passes"], b["visits"], b["converged"]), (case.id, i)
            assert a["support"] == b["support"], (case.id, i)
    if exact:
        np.testing.assert_allclose(got["r"], want["r"], rtol=0, atol=RESID_TOL, err_msg=case.id)


def check_design(case):
    """What a case is THERE for, asserted from the oracle's own supports (the kernel publishes no count of its own)."""
    want, d = oracle_of(case), data(case)
    nnz = [len(s["support"]) for s in want["solves"]]
    if case.max_iter > 3:
        assert all(s["converged"] for s in want["solves"]), case.id
    else:
        assert [(s["passes"], s["converged"]) for s in want["solves"]] == [(3, False)], case.id
    if case in MATRIX or case in WEIGHTED or case in F32:
        if case.p >= 128:
            assert nnz[0] <= 64 < nnz[-1], (case.id, nnz)              # the support crosses a chunk of 64 inside the path ...
        if case.p >= 256:
            assert nnz[-1] > SP.ncache(case.p), (case.id, nnz)         # ... and outgrows the column cache
        if case.p >= 65:
            hit = set(want["solves"][-1]["support"])
            assert {63, 64, 65, case.p} <= hit, (case.id, sorted(hit))  # movers on lane 63, on lane 0 of the next chunk, in the last valid lane
    if case in COLD or case in CUT:
        assert nnz[-1] > max(64, SP.ncache(case.p)), (case.id, nnz)
    if case in DROPZEROS:
        start = int(np.count_nonzero(d["x0"]))
        assert start == int(case.x0[5:]) and start > 64
        assert nnz[-1] == 6 if case.s == 6 else 64 < nnz[-1] < start, (case.id, nnz)
        if case.x0 == "small70":
            assert sorted(want["solves"][-1]["support"]) == [295, 296, 297, 298, 299, 300]
    if case in LONG_WARM:
        assert int(np.count_nonzero(d["x0"])) == 130 and nnz[-1] > 64, (case.id, nnz)
