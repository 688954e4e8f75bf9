#!/usr/bin/env python3
"""The fold-aware IRLS step against the plain one, and cvLogisticLassoPath against the same cross-validation composed from
the exports the library had before it.

 (a) cdh_glm_irls_fold(k, apply = 1) against cdh_glm_irls(apply = 1) on ONE fp64 handle (default n = 10 000 000, one column,
     K = 5 folds, k = 2): the fold step reads one byte per row more (49 bytes per row against 48).  Interleaved call by call,
     REPS calls each per round, ROUNDS rounds; reported are each round's minimum, the minimum and the spread of those over
     the rounds, and the ratio of the minima.  Times are host clocks around calls that end in a stream synchronise.
 (b) cvLogisticLassoPath (default n = 2 000 000, p = 1000, K = 5, 30 lambdas from 0.9 to 0.05 of lambda_max, IRLS optTol
     1e-7, full_path = False) against the same folds composed inside this tool from the exports before cdh_glm_irls_fold:
     per round cdh_get_residual, w and z in numpy with the held-out rows at w = 0 and z = eta, cdh_set_y,
     cdh_set_obs_weights and cdh_initialize, then the same solve; the held-out deviance from the same eta.  The two routes
     are interleaved on one handle, ROUNDS rounds after a warm-up of each; reported: wall times, their minima and spread,
     the IRLS rounds of each and the largest difference of fold_deviance.

Writes the report to OUT (default profiles/cv_logistic_shape.txt).  Environment: N, REPS, ROUNDS, N2, P2, K2, M2, OUT."""
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
n2, p2, K2, m2 = env("N2", 2_000_000), env("P2", 1000), env("K2", 5), env("M2", 30)
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "cv_logistic_shape.txt"))
lines = [f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; float64"]
print(lines[0], flush=True)
vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
WMIN = 1e-5


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def sigmoid(eta):
    e = np.exp(-np.abs(eta))
    return np.where(eta >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def logistic(n_, p_, seed, s):
    """A CDLogisticLoss on a design generated on the device: labels ~ Bernoulli(sigma(X beta* + noise))."""
    f, _ = cd.CDLogisticLoss.generate(n_, p_, seed=seed, s=s, noise=1.0)
    labels = (np.random.default_rng(seed).random(n_) < sigmoid(f.y)).astype(np.float64)
    cd.check(f._L.cdh_glm_set_labels(f._h, 0, vp(labels)), f._h)
    return f, labels


# ---- (a) the fold step against the plain step ------------------------------------------------------------------------------
f, _ = logistic(n, 1, 7, 1)
f.set_folds(np.random.default_rng(0).permutation(n) % 5, 5)
x = cd.SparseIterate(1)
x[1] = 2.0
cd.initialize_(f, x)                                                           # eta = 2 X_1: spread over about +-8
out3, out5 = np.zeros(3), np.zeros(5)
po3, po5 = out3.ctypes.data_as(C.POINTER(C.c_double)), out5.ctypes.data_as(C.POINTER(C.c_double))
plain = lambda: cd.check(f._L.cdh_glm_irls(f._h, 1, WMIN, po3), f._h)          # noqa: E731  (eta = z - r: the same every call)
fold = lambda: cd.check(f._L.cdh_glm_irls_fold(f._h, 2, 1, WMIN, po5), f._h)   # noqa: E731
nofold = lambda: cd.check(f._L.cdh_glm_irls_fold(f._h, -1, 1, WMIN, po5), f._h)  # noqa: E731
plain(), fold(), nofold()                                                      # warm-up of all three
per_round = {"cdh_glm_irls_apply1": [], "cdh_glm_irls_fold_apply1": [], "cdh_glm_irls_fold_k-1_apply1": []}
for _ in range(rounds):
    ta, tb, tc = [], [], []
    for _ in range(reps):
        ta.append(timed(plain)[0])
        tb.append(timed(fold)[0])
        tc.append(timed(nofold)[0])
    per_round["cdh_glm_irls_apply1"].append(min(ta))
    per_round["cdh_glm_irls_fold_apply1"].append(min(tb))
    per_round["cdh_glm_irls_fold_k-1_apply1"].append(min(tc))
fold()
held_rows = int(np.count_nonzero(f.w == 0.0))
f.close()
res = {"n": n, "K": 5, "k": 2, "held_out_rows": held_rows, "bytes_per_row": {"plain": 48, "fold": 49}}
for key, v in per_round.items():
    moved = (48 if key == "cdh_glm_irls_apply1" or "k-1" in key else 49) * n
    res[key] = {"round_minima_ms": [1e3 * t for t in v], "min_ms": 1e3 * min(v), "spread_ms": 1e3 * (max(v) - min(v)),
                "TBps": moved / min(v) / 1e12}
res["fold_over_plain"] = min(per_round["cdh_glm_irls_fold_apply1"]) / min(per_round["cdh_glm_irls_apply1"])
res["expected_at_most"] = 49.0 / 48.0
lines.append(json.dumps(res))
print(lines[-1], flush=True)

# ---- (b) the front end against the composed cross-validation ---------------------------------------------------------------
f, labels = logistic(n2, p2, 11, 10)
lmax = cd.logisticLambdaMax(f)
lam = lmax * np.geomspace(0.9, 0.05, m2)
opts = cd.CDOptions(maxIter=2000, optTol=1e-7, randomize=False)
irls = cd.IRLSOptions()
ids = (np.random.default_rng(0).permutation(n2) % K2).astype(np.int32)          # what cvLogisticLassoPath(seed=0) draws
sizes = np.bincount(ids, minlength=K2)


def device_route():
    return cd.cvLogisticLassoPath(f, None, lam, K=K2, seed=0, options=opts, irls=irls, full_path=False)


def composed_route():
    """The folds of cvLogisticLassoPath as the exports before cdh_glm_irls_fold allow them: three n-sized transfers and an
    initialize! per round, the fold's mask applied on the host."""
    L, h = f._L, f._h
    dev, rounds_, r = np.zeros((K2, m2)), 0, np.zeros(n2)
    mode = f.gradient_cache_mode()
    if mode == 1:
        f.set_gradient_cache(2)
    try:
        for k in range(K2):
            held = ids == k
            nk = n2 - sizes[k]
            cd.check(L.cdh_set_obs_weights(h, vp((~held).astype(np.float64))), h)
            sx = cd.stdX(f, weighted=True)
            x, z = cd.SparseIterate(p2), np.zeros(n2)
            cd.check(L.cdh_set_y(h, vp(z)), h)
            f._synced = None
            cd.initialize_(f, x)
            for j, lj in enumerate(lam):
                g, beta = cd.ProxL1(lj * np.sqrt(nk / n2), sx), x.dense()
                for _ in range(irls.maxIter):
                    cd.check(L.cdh_get_residual(h, vp(r)), h)
                    eta = z - r
                    e = np.exp(-np.abs(eta))
                    ope = 1.0 + e
                    pr = np.where(eta >= 0.0, 1.0 / ope, e / ope)
                    qr = np.where(eta >= 0.0, e / ope, 1.0 / ope)
                    w = np.where(held, 0.0, np.maximum(e / (ope * ope), irls.wmin))
                    z = np.where(held, eta, eta + (labels * qr - (1.0 - labels) * pr) / np.where(held, 1.0, w))
                    cd.check(L.cdh_set_y(h, vp(z)), h)
                    cd.check(L.cdh_set_obs_weights(h, vp(w)), h)
                    f._synced = None
                    cd.initialize_(f, x)
                    cd.coordinateDescent_(x, f, g, opts)
                    rounds_ += 1
                    beta, old = x.dense(), beta
                    if np.max(np.abs(beta - old)) < irls.optTol:
                        break
                cd.check(L.cdh_get_residual(h, vp(r)), h)                      # the held-out deviance at the solution
                eh = (z - r)[held]
                nll = (np.maximum(eh, 0.0) + np.log1p(np.exp(-np.abs(eh)))) - labels[held] * eh
                dev[k, j] = 2.0 * nll.sum() / sizes[k]
    finally:
        if mode == 1:
            f.set_gradient_cache(1)
    return dev, rounds_


device_route(), composed_route()                                               # warm-up of both
t_dev, t_com = [], []
for _ in range(rounds):
    t, cv = timed(device_route)
    t_dev.append(t)
    t, (cdev, crounds) = timed(composed_route)
    t_com.append(t)
f.close()
res = {"n": n2, "p": p2, "K": K2, "lambdas": m2, "cvLogisticLassoPath_s": t_dev, "composed_s": t_com,
       "min_s": {"cvLogisticLassoPath": min(t_dev), "composed": min(t_com)},
       "spread_s": {"cvLogisticLassoPath": max(t_dev) - min(t_dev), "composed": max(t_com) - min(t_com)},
       "composed_over_cvLogisticLassoPath": min(t_com) / min(t_dev),
       "irls_rounds": {"cvLogisticLassoPath": int(cv.rounds.sum()), "composed": int(crounds)},
       "n_sized_host_transfers_per_round": {"cvLogisticLassoPath": 0, "composed": 3},
       "index_min": int(cv.index_min), "index_1se": int(cv.index_1se),
       "max_abs_diff_fold_deviance": float(np.max(np.abs(cv.fold_deviance - cdev)))}
lines.append(json.dumps(res))
print(lines[-1], flush=True)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
