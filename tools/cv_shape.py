#!/usr/bin/env python3
"""The evaluation pass of cvLassoPath against its yardstick, and the front end against a cross-validation loop composed from
the exports the library had before it.

 (a) cdh_path_sse (k_path_sse) against cdh_xt_r_cols (k_col_dots) over the same S columns of ONE fp64 handle whose columns
     stream from HBM (default n = 2 000 000, S = 64 columns, M = 100 coefficient columns, 5 folds, fold 0 held out;
     generated on the device).  cdh_xt_r_cols streams the same column bytes once, so it is the yardstick.  The two are
     interleaved call by call, REPS calls each per round, ROUNDS rounds; reported are each round's minimum, the minimum and
     the spread of those over the rounds, the ratio, and the two roofline terms of the pass: the column bytes n sz S over
     the time, and the fp64 FMAs n S Mpad (Mpad: M rounded up to whole groups of kCvGroup, which is what the kernel
     executes) over the time.  Times are host clocks around calls that end in a stream synchronise and a small copy.
 (b) cvLassoPath (default n = 2 000 000, p = 1000, K = 5, 50 lambdas from 0.9 to 0.05 of lambda_max) against a loop composed
     inside this tool: per fold the 0/1 weights uploaded from the host (cdh_set_obs_weights), the same warm-started path,
     and after every lambda the held-out error read off the carried residual (cdh_resid_moments minus cdh_resid_wmoments),
     which makes the residual catch up once per solve.  Reported: wall time of each, the gradient cache's
     residual_catchups of each, and the largest relative difference of fold_mse.

Writes the report to OUT (default profiles/cv_shape.txt).  Environment: N, S, M, REPS, ROUNDS, N2, P2, K2, M2, OUT."""
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import coordinatedescent_jl_amd as cd  # noqa: E402

env = lambda k, d: int(os.environ.get(k, d))  # noqa: E731
n, s, m, reps, rounds = env("N", 2_000_000), env("S", 64), env("M", 100), env("REPS", 5), env("ROUNDS", 3)
n2, p2, K2, m2 = env("N2", 2_000_000), env("P2", 1000), env("K2", 5), env("M2", 50)
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "cv_shape.txt"))
plan = open(os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc", "cv_plan.hpp")).read()
G = int(re.search(r"constexpr\s+int\s+kCvGroup\s*=\s*(\d+)", plan).group(1))
lines = [f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; float64; kCvGroup={G}"]
print(lines[0], flush=True)
vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


# ---- (a) the pass against its yardstick ---------------------------------------------------------------------------------
f, _ = cd.CDLeastSquaresLoss.generate(n, s, seed=7, s=10, noise=1.0)
rng = np.random.default_rng(0)
f.set_folds(rng.permutation(n) % 5, 5)
idx1 = np.arange(1, s + 1, dtype=np.int64)
B = np.asfortranarray(rng.standard_normal((s, m)) * (rng.random((s, m)) < 0.5))
dots = np.zeros(s)
sse = lambda: f.path_sse(0, idx1, B)  # noqa: E731
xtr = lambda: cd.check(f._L.cdh_xt_r_cols(f._h, s, vp(idx1), vp(dots)), f._h)  # noqa: E731
sse(), xtr()                                                                   # warm-up of both
per_round = {"cdh_path_sse": [], "cdh_xt_r_cols": []}
for _ in range(rounds):
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(sse)[0])
        tb.append(timed(xtr)[0])
    per_round["cdh_path_sse"].append(min(ta))
    per_round["cdh_xt_r_cols"].append(min(tb))
f.close()
col_bytes, mpad = n * 8 * s, -(-m // G) * G
res = {"n": n, "s": s, "m": m, "mpad": mpad, "column_bytes": col_bytes, "fma": n * s * mpad}
for k, v in per_round.items():
    res[k] = {"round_minima_ms": [1e3 * t for t in v], "min_ms": 1e3 * min(v), "spread_ms": 1e3 * (max(v) - min(v)),
              "TBps_on_column_bytes": col_bytes / min(v) / 1e12}
res["cdh_path_sse"]["fp64_TFMAps"] = n * s * mpad / min(per_round["cdh_path_sse"]) / 1e12
res["cdh_path_sse"]["column_reads"] = mpad // G
res["path_sse_over_xt_r_cols"] = min(per_round["cdh_path_sse"]) / min(per_round["cdh_xt_r_cols"])
lines.append(json.dumps(res))
print(lines[-1], flush=True)

# ---- (b) the front end against the composed loop ------------------------------------------------------------------------
f, _ = cd.CDLeastSquaresLoss.generate(n2, p2, seed=11, s=10, noise=1.0)
cd.check(f._L.cdh_initialize(f._h, p2, 0, None, None), f._h)                   # beta = 0: r = y
xty = np.zeros(p2)
cd.check(f._L.cdh_xt_r(f._h, vp(xty)), f._h)
lam = np.max(np.abs(xty)) / n2 * np.geomspace(0.9, 0.05, m2)
opts = cd.CDOptions(maxIter=2000, optTol=1e-7, randomize=False)
ids = np.random.default_rng(0).permutation(n2) % K2                            # what cvLassoPath(seed=0) draws
sizes = np.bincount(ids, minlength=K2)


def composed():
    """The cross-validation loop as the exports before cdh_set_fold_weights / cdh_path_sse allow it."""
    L, h = f._L, f._h
    mse = np.zeros((K2, m2))
    cd.check(L.cdh_set_loss(h, cd.CDH_WLS), h)
    f._synced = None
    try:
        for k in range(K2):
            w = np.ascontiguousarray((ids != k).astype(np.float64))
            cd.check(L.cdh_set_obs_weights(h, vp(w)), h)
            f._synced = None
            nk = n2 - sizes[k]
            sx, x = cd.stdX(f, weighted=True), cd.SparseIterate(p2)
            cd.check(L.cdh_set_reuse_residual(h, 1), h)
            mode = f.gradient_cache_mode()
            if mode == 1:
                f.set_gradient_cache(2)
            try:
                for j, lj in enumerate(lam * np.sqrt(nk / n2)):
                    cd.coordinateDescent_(x, f, cd.ProxL1(lj, sx), opts)
                    a, aa, sw, swr = C.c_double(), C.c_double(), C.c_double(), C.c_double()
                    cd.check(L.cdh_resid_moments(h, C.byref(a), C.byref(aa)), h)
                    cd.check(L.cdh_resid_wmoments(h, C.byref(sw), C.byref(swr)), h)
                    mse[k, j] = (aa.value - swr.value) / sizes[k]
            finally:
                cd.check(L.cdh_set_reuse_residual(h, 0), h)
                if mode == 1:
                    f.set_gradient_cache(1)
    finally:
        cd.check(L.cdh_set_loss(h, cd.CDH_LS), h)
        f._synced = None
    return mse


def one_pass():
    return cd.cvLassoPath(f, None, lam, K=K2, seed=0, options=opts, full_path=False)


one_pass(), composed()                                                         # warm-up of both
c0 = f.cache_stats()["residual_catchups"]
t_cv, cv = timed(one_pass)
c1 = f.cache_stats()["residual_catchups"]
t_co, mse = timed(composed)
c2 = f.cache_stats()["residual_catchups"]
t_cv2, _ = timed(one_pass)
t_co2, _ = timed(composed)
f.close()
res = {"n": n2, "p": p2, "K": K2, "lambdas": m2, "cvLassoPath_s": [t_cv, t_cv2], "composed_s": [t_co, t_co2],
       "composed_over_cvLassoPath": min(t_co, t_co2) / min(t_cv, t_cv2),
       "residual_catchups": {"cvLassoPath": c1 - c0, "composed": c2 - c1},
       "max_rel_diff_fold_mse": float(np.max(np.abs(cv.fold_mse - mse) / np.abs(mse))),
       "index_min": cv.index_min, "index_1se": cv.index_1se}
lines.append(json.dumps(res))
print(lines[-1], flush=True)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
