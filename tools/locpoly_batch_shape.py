#!/usr/bin/env python3
"""cdh_vc_gram_batch against the per-point loop over cdh_vc_gram, on one handle, interleaved, ROUNDS rounds each after a
warm-up of both; the minimum and the spread (max - min) of each route are reported, and a route "wins" a shape only if its
minimum beats the other's by more than the larger of the two spreads.

 (a) grid: locpoly over 20 grid points at n = 1 000 000, p in {10, 50}, degree 1 and 2, fp64, Gaussian (the streamed regime;
     the shapes of profiles/locpoly_gram.txt, whose route A is the loop here);
 (b) leave-one-out: lvocv_locpoly at n = 2000, p = 10, degree 1, three bandwidths (the resident regime, 6000 points), device
     time (cdh_profile_begin/end: the kernels of the Gram exports) and wall time separately, so that the host's share --
     the solves and the copies -- is visible.

The loop routes are the front ends as they were before the batch export: one cdh_vc_gram and one scaled solve per point, and
for (b) one cdh_get_X_row per observation.  Times are host clocks around calls that end in a stream synchronise.  Writes the
report to OUT (default profiles/locpoly_batch.txt).  Environment: N, POINTS, N_LOO, ROUNDS, OUT."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import coordinatedescent_jl_amd as cd  # noqa: E402
from coordinatedescent_jl_amd.api import _solve_scaled, _vp  # noqa: E402

n, npoints, rounds = int(os.environ.get("N", 1_000_000)), int(os.environ.get("POINTS", 20)), int(os.environ.get("ROUNDS", 3))
n_loo = int(os.environ.get("N_LOO", 2000))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "locpoly_batch.txt"))
lines = [f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; rounds={rounds} float64; times in seconds"]
print(lines[0], flush=True)


def stat(v):
    return {"min": min(v), "max": max(v), "spread": max(v) - min(v)}


def verdict(batch, loop):
    margin = max(batch["spread"], loop["spread"])
    if loop["min"] - batch["min"] > margin:
        return "batch faster"
    if batch["min"] - loop["min"] > margin:
        return "loop faster"
    return "within the spread"


def timed(fn, f):
    f.profile_begin()
    t0 = time.perf_counter()
    out = fn(f)
    wall = time.perf_counter() - t0
    ms, launches, _ = f.profile_end()
    return wall, ms * 1e-3, launches, out


def compare(f, batch, loop, tag):
    batch(f), loop(f)                                                          # warm-up of both (and the scratch of both exports)
    wb, wl, db, dl, diff = [], [], [], [], 0.0
    for _ in range(rounds):
        a, da, la, oa = timed(batch, f)
        b, dbb, lb, ob = timed(loop, f)
        wb.append(a), wl.append(b), db.append(da), dl.append(dbb)
        diff = max(diff, float(np.max(np.abs(np.asarray(oa) - np.asarray(ob)))))
    sb, sl = stat(wb), stat(wl)
    res = dict(tag, batch_wall=sb, loop_wall=sl, batch_device=stat(db), loop_device=stat(dl), batch_launches=la, loop_launches=lb,
               loop_over_batch_wall_minima=sl["min"] / sb["min"], verdict_wall=verdict(sb, sl),
               verdict_device=verdict(stat(db), stat(dl)), max_abs_diff_of_results=diff)
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)


def data(nn, p):
    rng = np.random.default_rng(p)
    X = np.empty((nn, p), order="F")
    for j in range(p):
        X[:, j] = rng.standard_normal(nn)
    z = rng.random(nn)
    return X, z, np.sin(4 * z) * X[:, 0] + np.cos(6 * z) * X[:, 1] + 0.1 * rng.standard_normal(nn)


# ---- (a) the grid ------------------------------------------------------------------------------------------------------------
kernel, zgrid = cd.GaussianKernel(0.1), np.linspace(0.05, 0.95, npoints)


def grid_batch(f):
    G, c, _ = f.expanded_gram_batch(cd.GaussianKernel, kernel.h, zgrid)
    from coordinatedescent_jl_amd.api import _solve_scaled_stack
    return np.ascontiguousarray(_solve_scaled_stack(G, c).T)


def grid_loop(f):
    out = np.zeros((f.p, npoints))
    for ind, zz in enumerate(zgrid):
        G, c, _ = f.expanded_gram(kernel, zz)
        out[:, ind] = _solve_scaled(G, c)
    return out


for p in (10, 50):
    X, z, y = data(n, p)
    for deg in (1, 2):
        f = cd.CDVaryingCoefficientLoss(y, X, z, deg)
        compare(f, grid_batch, grid_loop, {"shape": "grid", "n": n, "p": p, "degree": deg, "points": npoints})
        f.close()
    del X, z, y

# ---- (b) leave-one-out ---------------------------------------------------------------------------------------------------------
hs = [0.1, 0.2, 0.4]


def loo_batch(f):
    from coordinatedescent_jl_amd.api import _locpoly_batch
    Q1, nn = f.degree + 1, f.n
    yv = f.y.astype(np.float64)
    Xb = np.concatenate([f.X_cols(j * Q1, 1) for j in range(f.p_base)], axis=1).astype(np.float64)
    pair = np.arange(len(hs) * nn)
    indH, obs = pair // nn, pair % nn
    hbeta = _locpoly_batch(f, 0, np.asarray(hs)[indH], None, obs)
    sq = (np.einsum("ij,ij->i", Xb[obs], hbeta[:, ::Q1]) - yv[obs]) ** 2
    MSE = np.zeros(len(hs))
    for k, v in zip(indH.tolist(), sq.tolist()):
        MSE[k] += v
    return MSE


def loo_loop(f):
    Q1 = f.degree + 1
    yv = f.y.astype(np.float64)
    base = np.ascontiguousarray(np.arange(f.p_base, dtype=np.int64) * Q1 + 1)
    xrow = np.zeros(f.p_base)
    MSE = np.zeros(len(hs))
    for indH, h in enumerate(hs):
        k = cd.GaussianKernel(h)
        for i in range(f.n):
            G, c, _ = f.expanded_gram(k, leave_out=i)
            hbeta = _solve_scaled(G, c)
            cd.check(f._L.cdh_get_X_row(f._h, i, f.p_base, _vp(base), _vp(xrow)), f._h)
            MSE[indH] += (float(xrow @ hbeta[::Q1]) - yv[i]) ** 2
    return MSE


X, z, y = data(n_loo, 10)
f = cd.CDVaryingCoefficientLoss(y, X, z, 1)
compare(f, loo_batch, loo_loop, {"shape": "leave-one-out", "n": n_loo, "p": 10, "degree": 1, "bandwidths": hs, "points": len(hs) * n_loo})
f.close()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
