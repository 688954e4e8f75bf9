#!/usr/bin/env python3
"""The IRLS step of the Poisson lasso against its yardsticks, and the front end against the same loop composed from the exports
the library had before it.

 (a) cdh_glm_poisson_irls(apply = 1) with an offset and a fold held out -- and apply = 0 -- on ONE fp64 handle (default
     n = 10 000 000, one column) against (i) a device-to-device copy of the bytes it moves and (ii) the fold-aware binomial
     step cdh_glm_irls_fold(apply = 1) on a handle of the same shape.  The Poisson step reads four n-vectors (counts, y, r,
     offset) and a byte per row and writes three (w, y, r): 57 bytes a row, against the binomial step's 49.  The copy moves
     the same 57 n bytes: three vectors of n doubles, one of n / 2 doubles and n / 2 bytes, read and written.
     THE EXPECTATION, stated before the run: both steps stream, so the Poisson step takes the binomial step's time x 57 / 49
     (= 1.163); it is reported as met when the measured ratio is within the spread of the rounds' minima (as a share of the
     minimum) above that, and as missed otherwise.  Interleaved call by call, REPS calls each per round, ROUNDS rounds;
     reported are each round's minimum, the minimum and the spread of those over the rounds, and the bytes over the time.
     Times are host clocks around calls that end in a stream synchronise (a step also brings back its sums).
 (b) PoissonLassoPath (default n = 2 000 000, p = 1000, 30 lambdas from 0.9 to 0.05 of lambda_max, with an offset, IRLS optTol
     1e-7) against the same warm-started loop composed inside this tool from what the library offered before: a weighted
     least-squares handle, per round cdh_get_residual, mu, w and z in numpy (the formulas of tests/_poisson_numpy.py),
     cdh_set_y, cdh_set_obs_weights and cdh_initialize, then the same solve.  The two routes are interleaved on one handle,
     ROUNDS rounds after a warm-up of each; reported: wall times, their minima and spread, the IRLS rounds of each (they must
     be equal), the n-sized host transfers per round of each, and the largest difference of the coefficients.

WEIGHTS=1: the same with observation weights (log-uniform over [0.25, 4], normalised to sum to n; cdh_glm_set_weights).
 (a) gains the Poisson step on a handle of the same shape WITH weights: the same kernel with one more 16-byte stream, 65
     bytes a row against 57.  THE EXPECTATION, stated before the run: both stream, so the weighted step takes the
     unweighted one's time x 65 / 57 (= 1.140); met when the measured ratio is within the spread of the rounds' minima (as a
     share of the minimum) above that, missed otherwise.
 (b) becomes PoissonLassoPath on the loss with weights against the composed loop with v w for w.
The report is then APPENDED to OUT (default profiles/glm_weights_timing.txt, which tools/logistic_shape.py shares).

Writes the report to OUT (default profiles/poisson_shape.txt).  Environment: N, REPS, ROUNDS, N2, P2, M2, OUT, WEIGHTS."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import coordinatedescent_jl_amd as cd  # noqa: E402

env = lambda k, d: int(os.environ.get(k, d))  # noqa: E731
n, reps, rounds = env("N", 10_000_000), env("REPS", 5), env("ROUNDS", 3)
n2, p2, m2 = env("N2", 2_000_000), env("P2", 1000), env("M2", 30)
weighted = env("WEIGHTS", 0) == 1
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "glm_weights_timing.txt" if weighted else "poisson_shape.txt"))
lines = [f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; float64"]
if weighted:
    lines.insert(0, "== tools/poisson_shape.py WEIGHTS=1 ==")
print(lines[0], flush=True)
vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
PD = C.POINTER(C.c_double)
WMIN, ETA_MAX, K = 1e-5, 50.0, 10


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def poisson(n_, p_, seed, s):
    """A CDPoissonLoss on a design generated on the device: o = log U(.5, 2), counts ~ Poisson(exp(eta* + o)) with eta* the
    generated signal scaled to a standard deviation of one half."""
    f, _ = cd.CDPoissonLoss.generate(n_, p_, seed=seed, s=s, noise=1.0)
    rng = np.random.default_rng(seed)
    sig = f.y
    o = np.log(rng.uniform(0.5, 2.0, n_))
    counts = rng.poisson(np.exp(0.5 * sig / np.std(sig) + o)).astype(np.float64)
    cd.check(f._L.cdh_glm_set_counts(f._h, vp(counts), vp(o)), f._h)
    return f, counts, o


def set_weights(f, seed):
    """Log-uniform weights over [0.25, 4], normalised to sum to n, on a loss made by generate (what weights= does)."""
    v = np.exp(np.random.default_rng(100 + seed).uniform(np.log(0.25), np.log(4.0), f.n))
    v *= f.n / v.sum()
    cd.check(f._L.cdh_glm_set_weights(f._h, vp(v)), f._h)
    f._has_weights = True
    return v


# ---- (a) the step against the copy of its bytes and against the binomial step --------------------------------------------
f, _, _ = poisson(n, 1, 7, 1)
g, _ = cd.CDLogisticLoss.generate(n, 1, seed=7, s=1, noise=1.0)
labels = (np.random.default_rng(7).random(n) < 0.5).astype(np.float64)
cd.check(g._L.cdh_glm_set_labels(g._h, 0, vp(labels)), g._h)
ids = (np.arange(n) % K).astype(np.int32)
x = cd.SparseIterate(1)
x[1] = 2.0
fw = None
if weighted:
    fw, _, _ = poisson(n, 1, 7, 1)
    set_weights(fw, 7)
for h in (f, g) + ((fw,) if weighted else ()):
    h.set_folds(ids, K)
    cd.initialize_(h, x)                                                       # eta_lin = 2 X_1: spread over about +-8
out6, out5 = np.zeros(6), np.zeros(5)
pois1 = lambda: cd.check(f._L.cdh_glm_poisson_irls(f._h, 0, 1, WMIN, ETA_MAX, out6.ctypes.data_as(PD)), f._h)  # noqa: E731
pois0 = lambda: cd.check(f._L.cdh_glm_poisson_irls(f._h, 0, 0, WMIN, ETA_MAX, out6.ctypes.data_as(PD)), f._h)  # noqa: E731
binom1 = lambda: cd.check(g._L.cdh_glm_irls_fold(g._h, 0, 1, WMIN, out5.ctypes.data_as(PD)), g._h)            # noqa: E731
src = [torch.randn(n, dtype=torch.float64, device="cuda") for _ in range(3)] + [
    torch.randn(n // 2, dtype=torch.float64, device="cuda"), torch.zeros(n // 2, dtype=torch.uint8, device="cuda")]
dst = [torch.empty_like(a) for a in src]
copied = 2 * sum(a.numel() * a.element_size() for a in src)


def copy57():
    for a, b in zip(src, dst):
        b.copy_(a)
    torch.cuda.synchronize()


pois1(), pois0(), binom1(), copy57()                                           # warm-up of all four
names = ("cdh_glm_poisson_irls_apply1", "cdh_glm_poisson_irls_apply0", "cdh_glm_irls_fold_apply1", "copy_57_bytes_a_row")
fns = (pois1, pois0, binom1, copy57)
if weighted:
    out6w = np.zeros(6)
    wpois1 = lambda: cd.check(fw._L.cdh_glm_poisson_irls(fw._h, 0, 1, WMIN, ETA_MAX, out6w.ctypes.data_as(PD)), fw._h)  # noqa: E731
    wpois0 = lambda: cd.check(fw._L.cdh_glm_poisson_irls(fw._h, 0, 0, WMIN, ETA_MAX, out6w.ctypes.data_as(PD)), fw._h)  # noqa: E731
    wpois1(), wpois0()
    names += ("weighted_poisson_irls_apply1", "weighted_poisson_irls_apply0")
    fns += (wpois1, wpois0)
per_round = {k: [] for k in names}
for _ in range(rounds):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn)[0])
    for k, t in zip(names, ts):
        per_round[k].append(min(t))
f.close()
g.close()
del src, dst
moved = {names[0]: 57 * n, names[1]: 33 * n, names[2]: 49 * n, names[3]: copied}
if weighted:
    fw.close()
    moved.update({names[4]: 65 * n, names[5]: 41 * n})
res = {"n": n, "bytes_a_row": {"poisson_apply1": 57, "poisson_apply0": 33, "binomial_fold_apply1": 49, "copy": copied / n},
       "clamped_rows": int(out6[2]), "capped_rows": int(out6[3])}
for k, v in per_round.items():
    res[k] = {"round_minima_ms": [1e3 * t for t in v], "min_ms": 1e3 * min(v), "spread_ms": 1e3 * (max(v) - min(v)),
              "TBps": moved[k] / min(v) / 1e12}
ratio = min(per_round[names[0]]) / min(per_round[names[2]])
slack = max((max(v) - min(v)) / min(v) for v in (per_round[names[0]], per_round[names[2]]))
res["poisson_over_copy"] = min(per_round[names[0]]) / min(per_round[names[3]])
res["poisson_over_binomial_fold"] = ratio
res["expected_poisson_over_binomial_fold"] = 57 / 49
res["expectation"] = "met" if ratio <= 57 / 49 * (1.0 + slack) else "missed"
if weighted:
    wratio = min(per_round[names[4]]) / min(per_round[names[0]])
    wslack = max((max(v) - min(v)) / min(v) for v in (per_round[names[0]], per_round[names[4]]))
    res["weighted_over_unweighted"] = wratio
    res["expected_weighted_over_unweighted"] = 65 / 57
    res["weighted_expectation"] = "met" if wratio <= 65 / 57 * (1.0 + wslack) else "missed"
lines.append(json.dumps(res))
print(lines[-1], flush=True)

# ---- (b) the front end against the composed loop ------------------------------------------------------------------------
f, counts, o = poisson(n2, p2, 11, 10)
v_obs = set_weights(f, 11) if weighted else 1.0
lmax = cd.poissonLambdaMax(f)
lam = lmax * np.geomspace(0.9, 0.05, m2)
opts = cd.CDOptions(maxIter=2000, optTol=1e-7, randomize=False)
irls = cd.IRLSOptions()
sx = cd.stdX(f)


def device_route():
    return cd.PoissonLassoPath(f, None, lam, opts, irls)


def composed_route():
    """PoissonLassoPath's loop as the exports before cdh_glm_poisson_irls allow it: three n-sized transfers and an initialize!
    per round, on the handle as the weighted least-squares loss it is."""
    L, h = f._L, f._h
    x, betas, rounds_, r = cd.SparseIterate(p2), [], [], np.zeros(n2)
    z = np.zeros(n2)
    cd.check(L.cdh_set_y(h, vp(z)), h)
    f._synced = None
    cd.initialize_(f, x)
    mode = f.gradient_cache_mode()
    if mode == 1:
        f.set_gradient_cache(2)
    try:
        for lj in lam:
            g_, beta, k = cd.ProxL1(lj, sx), x.dense(), 0
            for k in range(1, irls.maxIter + 1):
                cd.check(L.cdh_get_residual(h, vp(r)), h)
                eta_lin = z - r
                mu = np.exp(np.minimum(eta_lin + o, irls.etaMax))
                w = np.maximum(mu, irls.wmin)
                z = eta_lin + (counts - mu) / w
                w = v_obs * w if weighted else w
                cd.check(L.cdh_set_y(h, vp(z)), h)
                cd.check(L.cdh_set_obs_weights(h, vp(w)), h)
                f._synced = None
                cd.initialize_(f, x)
                cd.coordinateDescent_(x, f, g_, opts)
                beta, old = x.dense(), beta
                if np.max(np.abs(beta - old)) < irls.optTol:
                    break
            betas.append(beta)
            rounds_.append(k)
    finally:
        if mode == 1:
            f.set_gradient_cache(1)
    return betas, rounds_


device_route(), composed_route()                                               # warm-up of both
t_dev, t_com = [], []
for _ in range(rounds):
    t, path = timed(device_route)
    t_dev.append(t)
    t, (betas, crounds) = timed(composed_route)
    t_com.append(t)
f.close()
diff = max(float(np.max(np.abs(b.dense() - c))) for b, c in zip(path.betapath, betas))
res = {"n": n2, "p": p2, "lambdas": m2, "weights": weighted, "PoissonLassoPath_s": t_dev, "composed_s": t_com,
       "min_s": {"PoissonLassoPath": min(t_dev), "composed": min(t_com)},
       "spread_s": {"PoissonLassoPath": max(t_dev) - min(t_dev), "composed": max(t_com) - min(t_com)},
       "composed_over_PoissonLassoPath": min(t_com) / min(t_dev),
       "irls_rounds": {"PoissonLassoPath": int(sum(path.rounds)), "composed": int(sum(crounds))},
       "same_rounds_per_lambda": list(path.rounds) == list(crounds),
       "n_sized_host_transfers_per_round": {"PoissonLassoPath": 0, "composed": 3},
       "nnz_last": int(path.betapath[-1].nnz), "max_abs_diff_beta": diff}
lines.append(json.dumps(res))
print(lines[-1], flush=True)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "a" if weighted else "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
