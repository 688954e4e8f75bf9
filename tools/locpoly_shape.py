#!/usr/bin/env python3
"""locpolyl1 over a grid of points at a shape where the expanded design is several GB (default n = 1 000 000,
p_base = 500, degree 1, fp64, Gaussian kernel, 20 grid points; data generated on the host once):

 1. per grid point, the HIP-event time of k_vc_weights + k_vc_expand + k_vc_reduce (cdh_profile_begin / _end around
    cdh_vc_set_point) and the rate on the algorithmic bytes n sz (p (q + 1) + 2); alongside, in the same process, a
    device-to-device copy of n sz p q bytes (what the expansion writes) as the yardstick of a read-one-write-one stream;
 2. the whole locpolyl1, device expansion (route A) against the route the C ABI offered before it (route B: numpy expansion,
    weights and weighted column scales on the host, cdh_set_X_cols + cdh_set_obs_weights per point, the same solves),
    interleaved A/B, the coefficients of the two compared.  GATE: A is faster than B, and faster than B's uploads and
    solves alone (its host arithmetic left out);
 3. cache_stats / onchip_stats of both handles, for information.

Environment: N, PB, DEG, POINTS, REPS (timed repeats per point, default 10), ROUNDS (A/B rounds, default 2), DTYPE (f64 / f32)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import coordinatedescent_jl_amd as cd  # noqa: E402
from coordinatedescent_jl_amd.api import _vp  # noqa: E402

n, pb, deg = int(os.environ.get("N", 1_000_000)), int(os.environ.get("PB", 500)), int(os.environ.get("DEG", 1))
npoints, reps, rounds = int(os.environ.get("POINTS", 20)), int(os.environ.get("REPS", 10)), int(os.environ.get("ROUNDS", 2))
dtype = np.float32 if os.environ.get("DTYPE", "f64") == "f32" else np.float64
sz, ep = np.dtype(dtype).itemsize, pb * (deg + 1)
kernel, lam0 = cd.GaussianKernel(0.05), 0.02
opt = cd.CDOptions(maxIter=2000, optTol=1e-8, randomize=False)
zgrid = np.linspace(0.05, 0.95, npoints)
print(f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; n={n} p_base={pb} degree={deg} "
      f"{np.dtype(dtype).name} points={npoints} reps={reps} rounds={rounds}", flush=True)

rng = np.random.default_rng(2024)
t0 = time.perf_counter()
X = np.empty((n, pb), dtype=dtype, order="F")
for j in range(pb):
    X[:, j] = rng.standard_normal(n)
z = rng.random(n).astype(dtype)
s = min(10, pb)
y = ((np.sin(z[:, None].astype(np.float64) * rng.choice([2, 4, 6, 8], size=s)) * X[:, :s]).sum(axis=1)
     + 0.1 * rng.standard_normal(n)).astype(dtype)
print(f"host data generated in {time.perf_counter() - t0:.1f} s", flush=True)


def spread(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1]}


# ---- 1. the expansion kernels per grid point, and the copy yardstick -------------------------------------------------
fA = cd.CDVaryingCoefficientLoss(y, X, z, deg)
alg_bytes = n * sz * (ep + 2)
for z0 in zgrid[:2]:
    fA.set_point(kernel, z0)                                      # warm-up
per_point = []
for z0 in zgrid:
    ms = []
    for _ in range(reps):
        fA.profile_begin()
        fA.set_point(kernel, z0)
        t, _, b = fA.profile_end()
        assert b == alg_bytes, (b, alg_bytes)
        ms.append(t)
    per_point.append(statistics.median(ms))
    print(f"  z0={z0:.3f}: set_point kernels {spread(ms)} ms", flush=True)
copy_bytes = n * sz * pb * max(deg, 1)
src = torch.empty(copy_bytes // 8, dtype=torch.float64, device="cuda").normal_()
dst = torch.empty_like(src)
for _ in range(3):
    dst.copy_(src)
torch.cuda.synchronize()
copy_ms = []
for _ in range(max(reps, 10)):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    copy_ms.append(e0.elapsed_time(e1))
del src, dst
torch.cuda.empty_cache()
exp_ms, cp = spread(per_point), spread(copy_ms)
res = {"expand_ms_per_point": exp_ms, "algorithmic_bytes": alg_bytes, "expand_GBps": alg_bytes / exp_ms["median"] / 1e6,
       "d2d_copy_bytes": copy_bytes, "d2d_copy_ms": cp, "d2d_copy_GBps_read_plus_write": 2 * copy_bytes / cp["median"] / 1e6,
       "expand_ms_over_copy_ms": exp_ms["median"] / cp["median"]}
print(json.dumps(res), flush=True)

# ---- 2. the whole grid: device expansion (A) against host expansion + uploads (B) --------------------------------------
fB = cd.CDWeightedLSLoss.__new__(cd.CDWeightedLSLoss)
fB._create(dtype, n, ep, 0, None, 0)
cd.check(fB._L.cdh_set_y(fB._h, _vp(np.ascontiguousarray(y))), fB._h)
eX = np.empty((n, ep), dtype=dtype, order="F")
eX[:, ::deg + 1] = X


def route_a():
    fA.point_stats.clear()
    t0 = time.perf_counter()
    out, _ = cd.locpolyl1(fA, None, None, zgrid, deg, kernel, lam0, False, opt)
    return time.perf_counter() - t0, out, {}


def route_b():
    inner = cd.CDOptions(opt.maxIter, opt.optTol, opt.randomize, True, opt.numSteps, opt.seed)
    beta, out = cd.SparseIterate(ep), np.zeros((ep, npoints))
    t_host = t_up = 0.0
    t0 = time.perf_counter()
    for i, z0 in enumerate(zgrid):
        th = time.perf_counter()
        w = cd.evaluate(kernel, z.astype(np.float64), z0).astype(dtype)
        df = z - dtype(z0)
        for l in range(1, deg + 1):
            np.multiply(eX[:, l - 1::deg + 1], df[:, None], out=eX[:, l::deg + 1])
        sx = np.sqrt(np.array([np.dot(w * eX[:, j], eX[:, j]) for j in range(ep)], dtype=np.float64) / n)
        tu = time.perf_counter()
        cd.check(fB._L.cdh_set_X_cols(fB._h, 0, ep, _vp(eX), n), fB._h)
        cd.check(fB._L.cdh_set_obs_weights(fB._h, _vp(w)), fB._h)
        ts = time.perf_counter()
        t_host, t_up = t_host + (tu - th), t_up + (ts - tu)
        cd.coordinateDescent_(beta, fB, cd.ProxL1(lam0, sx), inner)
        out[:, i] = beta.dense()
    total = time.perf_counter() - t0
    return total, out, {"host_arithmetic_s": t_host, "upload_s": t_up, "solve_s": total - t_host - t_up}


runs = {"A": [], "B": []}
for r in range(rounds):
    for name, fn in (("A", route_a), ("B", route_b)):
        t, out, extra = fn()
        runs[name].append((t, out, extra))
        print(f"  round {r} route {name}: {t:.3f} s {json.dumps(extra)}", flush=True)
tA, tB = spread([t for t, _, _ in runs["A"]]), spread([t for t, _, _ in runs["B"]])
tB_dev = spread([e["upload_s"] + e["solve_s"] for _, _, e in runs["B"]])
dbeta = float(np.max(np.abs(runs["A"][-1][1] - runs["B"][-1][1])))
res = {"locpolyl1_device_expansion_s": tA, "locpolyl1_host_expansion_s": tB, "host_route_uploads_and_solves_only_s": tB_dev,
       "speedup": tB["median"] / tA["median"], "speedup_over_uploads_and_solves_only": tB_dev["median"] / tA["median"],
       "max_abs_dbeta_between_routes": dbeta, "nnz_last_point": int(np.count_nonzero(runs["A"][-1][1][:, -1])),
       "passes_per_point_A": [s_["passes"] for s_ in fA.point_stats],
       "A": {"cache": fA.cache_stats(), "onchip": fA.onchip_stats()}, "B": {"cache": fB.cache_stats(), "onchip": fB.onchip_stats()}}
print(json.dumps(res), flush=True)
assert all(s_["converged"] for s_ in fA.point_stats)
assert dbeta <= 1e-10 or dtype == np.float32, dbeta
assert tA["max"] < tB["min"], "GATE: the device route must be faster than host expansion + uploads"
assert tA["max"] < tB_dev["min"], "GATE: ... and faster than that route's uploads and solves alone"
print("GATE met: device expansion is faster", flush=True)
