#!/usr/bin/env python3
"""The IRLS step of the logistic lasso against its yardstick, and the front end against the same loop composed from the
exports the library had before it.

 (a) cdh_glm_irls(apply = 1) -- and apply = 0 -- on ONE fp64 handle (default n = 10 000 000, one column) against a
     device-to-device copy of the same bytes: the step reads three n-vectors (labels, y, r) and writes three (w, y, r), so
     the yardstick is three copies of n doubles.  Interleaved call by call, REPS calls each per round, ROUNDS rounds;
     reported are each round's minimum, the minimum and the spread of those over the rounds, and the bytes over the time.
     Times are host clocks around calls that end in a stream synchronise (the step also brings back three doubles).
 (b) LogisticLassoPath (default n = 2 000 000, p = 1000, 30 lambdas from 0.9 to 0.05 of lambda_max, IRLS optTol 1e-7) against
     the same warm-started loop composed inside this tool: per round cdh_get_residual, w and z in numpy (the formulas of
     tests/_logistic_numpy.py), cdh_set_y, cdh_set_obs_weights and cdh_initialize, then the same solve.  The two routes are
     interleaved on one handle, ROUNDS rounds after a warm-up of each; reported: wall times, their minima and spread, the
     IRLS rounds of each, the n-sized host transfers per round of each, and the largest difference of the coefficients.

WEIGHTS=1: the same with observation weights (log-uniform over [0.25, 4], normalised to sum to n; cdh_glm_set_weights).
 (a) becomes the fold-aware step cdh_glm_irls_fold(apply = 1), fold 0 of 10 held out, on a handle WITH weights against the
     same step on a handle of the same shape WITHOUT: the same kernel with one more 16-byte stream, 57 bytes a row against
     49.  THE EXPECTATION, stated before the run: both stream, so the ratio is 57 / 49 (= 1.163); met when the measured
     ratio is within the spread of the rounds' minima (as a share of the minimum) above that, missed otherwise.
 (b) becomes LogisticLassoPath on the loss with weights against the composed loop with v w for w.
The report is then APPENDED to OUT (default profiles/glm_weights_timing.txt, which tools/poisson_shape.py shares).

Writes the report to OUT (default profiles/logistic_shape.txt).  Environment: N, REPS, ROUNDS, N2, P2, M2, OUT, WEIGHTS."""
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
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "glm_weights_timing.txt" if weighted else "logistic_shape.txt"))
lines = [f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; float64"]
if weighted:
    lines.insert(0, "== tools/logistic_shape.py WEIGHTS=1 ==")
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


def set_weights(f, seed):
    """Log-uniform weights over [0.25, 4], normalised to sum to n, on a loss made by generate (what weights= does)."""
    v = np.exp(np.random.default_rng(100 + seed).uniform(np.log(0.25), np.log(4.0), f.n))
    v *= f.n / v.sum()
    cd.check(f._L.cdh_glm_set_weights(f._h, vp(v)), f._h)
    f._has_weights = True
    return v


def weighted_fold_step():
    """(a) with WEIGHTS=1: the fold-aware step with and without weights, interleaved."""
    K = 10
    ids = (np.arange(n) % K).astype(np.int32)
    x = cd.SparseIterate(1)
    x[1] = 2.0
    hs = []
    for with_v in (False, True):
        h, _ = logistic(n, 1, 7, 1)
        if with_v:
            set_weights(h, 7)
        h.set_folds(ids, K)
        cd.initialize_(h, x)
        hs.append(h)
    out5 = np.zeros(5)
    p5 = out5.ctypes.data_as(C.POINTER(C.c_double))
    fns = [lambda h=h, a=a: cd.check(h._L.cdh_glm_irls_fold(h._h, 0, a, WMIN, p5), h._h) for h in hs for a in (1, 0)]
    names = ("fold_apply1", "fold_apply0", "weighted_fold_apply1", "weighted_fold_apply0")
    for fn in fns:
        fn()
    per = {k: [] for k in names}
    for _ in range(rounds):
        ts = [[] for _ in fns]
        for _ in range(reps):
            for t, fn in zip(ts, fns):
                t.append(timed(fn)[0])
        for k, t in zip(names, ts):
            per[k].append(min(t))
    for h in hs:
        h.close()
    bytes_a_row = dict(zip(names, (49, 25, 57, 33)))
    res = {"n": n, "bytes_a_row": bytes_a_row}
    for k, v in per.items():
        res[k] = {"round_minima_ms": [1e3 * t for t in v], "min_ms": 1e3 * min(v), "spread_ms": 1e3 * (max(v) - min(v)),
                  "TBps": bytes_a_row[k] * n / min(v) / 1e12}
    ratio = min(per[names[2]]) / min(per[names[0]])
    slack = max((max(v) - min(v)) / min(v) for v in (per[names[0]], per[names[2]]))
    res["weighted_over_unweighted"] = ratio
    res["expected_weighted_over_unweighted"] = 57 / 49
    res["expectation"] = "met" if ratio <= 57 / 49 * (1.0 + slack) else "missed"
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)


# ---- (a) the step against the copy of its bytes ---------------------------------------------------------------------------
if weighted:
    weighted_fold_step()
f, _ = logistic(n, 1, 7, 1)
x = cd.SparseIterate(1)
x[1] = 2.0
cd.initialize_(f, x)                                                           # eta = 2 X_1: spread over about +-8
out3 = np.zeros(3)
po = out3.ctypes.data_as(C.POINTER(C.c_double))
step1 = lambda: cd.check(f._L.cdh_glm_irls(f._h, 1, WMIN, po), f._h)           # noqa: E731  (eta = z - r: the same every call)
step0 = lambda: cd.check(f._L.cdh_glm_irls(f._h, 0, WMIN, po), f._h)           # noqa: E731
src = [torch.randn(n, dtype=torch.float64, device="cuda") for _ in range(3)]
dst = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3)]


def copy3():
    for a, b in zip(src, dst):
        b.copy_(a)
    torch.cuda.synchronize()


step1(), step0(), copy3()                                                      # warm-up of all three
per_round = {"cdh_glm_irls_apply1": [], "cdh_glm_irls_apply0": [], "copy_3_vectors": []}
for _ in range(rounds):
    ta, tb, tc = [], [], []
    for _ in range(reps):
        ta.append(timed(step1)[0])
        tb.append(timed(step0)[0])
        tc.append(timed(copy3)[0])
    per_round["cdh_glm_irls_apply1"].append(min(ta))
    per_round["cdh_glm_irls_apply0"].append(min(tb))
    per_round["copy_3_vectors"].append(min(tc))
f.close()
del src, dst
res = {"n": n, "bytes_read_and_written": 6 * 8 * n, "clamped_rows": int(out3[2])}
for k, v in per_round.items():
    moved = (3 if k.endswith("apply0") else 6) * 8 * n
    res[k] = {"round_minima_ms": [1e3 * t for t in v], "min_ms": 1e3 * min(v), "spread_ms": 1e3 * (max(v) - min(v)),
              "TBps": moved / min(v) / 1e12}
res["apply1_over_copy"] = min(per_round["cdh_glm_irls_apply1"]) / min(per_round["copy_3_vectors"])
lines.append(json.dumps(res))
print(lines[-1], flush=True)

# ---- (b) the front end against the composed loop ------------------------------------------------------------------------
f, labels = logistic(n2, p2, 11, 10)
v_obs = set_weights(f, 11) if weighted else 1.0
lmax = cd.logisticLambdaMax(f)
lam = lmax * np.geomspace(0.9, 0.05, m2)
opts = cd.CDOptions(maxIter=2000, optTol=1e-7, randomize=False)
irls = cd.IRLSOptions()
sx = cd.stdX(f)


def device_route():
    return cd.LogisticLassoPath(f, None, lam, opts, irls)


def composed_route():
    """LogisticLassoPath's loop as the exports before cdh_glm_irls allow it: three n-sized transfers and an initialize! per
    round."""
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
            g, beta, k = cd.ProxL1(lj, sx), x.dense(), 0
            for k in range(1, irls.maxIter + 1):
                cd.check(L.cdh_get_residual(h, vp(r)), h)
                eta = z - r
                e = np.exp(-np.abs(eta))
                ope = 1.0 + e
                pr = np.where(eta >= 0.0, 1.0 / ope, e / ope)
                qr = np.where(eta >= 0.0, e / ope, 1.0 / ope)
                w = np.maximum(e / (ope * ope), irls.wmin)
                z = eta + (labels * qr - (1.0 - labels) * pr) / w
                w = v_obs * w if weighted else w
                cd.check(L.cdh_set_y(h, vp(z)), h)
                cd.check(L.cdh_set_obs_weights(h, vp(w)), h)
                f._synced = None
                cd.initialize_(f, x)
                cd.coordinateDescent_(x, f, g, opts)
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
res = {"n": n2, "p": p2, "lambdas": m2, "weights": weighted, "LogisticLassoPath_s": t_dev, "composed_s": t_com,
       "min_s": {"LogisticLassoPath": min(t_dev), "composed": min(t_com)},
       "spread_s": {"LogisticLassoPath": max(t_dev) - min(t_dev), "composed": max(t_com) - min(t_com)},
       "composed_over_LogisticLassoPath": min(t_com) / min(t_dev),
       "irls_rounds": {"LogisticLassoPath": int(sum(path.rounds)), "composed": int(sum(crounds))},
       "n_sized_host_transfers_per_round": {"LogisticLassoPath": 0, "composed": 3},
       "nnz_last": int(path.betapath[-1].nnz), "max_abs_diff_beta": diff}
lines.append(json.dumps(res))
print(lines[-1], flush=True)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "a" if weighted else "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
