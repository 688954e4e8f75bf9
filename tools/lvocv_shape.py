#!/usr/bin/env python3
"""lvocv_locpolyl1's loop at a shape where a point's setup is a real pass over the design (default n = 200 000, p_base = 20,
degree 1, fp64, Gaussian kernel, two bandwidths, the first ROWS = 100 observations of each: n points per bandwidth is the
reference's loop, a prefix of it is what can be timed), the new route against the only one the C ABI offered before it:

 A. cdh_vc_set_point_loo per point (weights with the left-out row, expansion, scales and screening scores on the device);
 B. numpy weights with the zeroed entry and numpy expansion, then cdh_set_X_cols + cdh_set_obs_weights, and the scales and
    scores from the device calls that existed already (cdh_col_wrms; cdh_initialize with the zero iterate + cdh_xt_r_cols);

with the same calls after that on both (api._lvocv_point: screening init, sigma loop, refit, prediction).  Interleaved A/B
after a warm-up round; per route the split between point setup and the rest; the squared errors of the two compared.  The CPU
oracle (tests/_vc_cv_numpy.py through `oracle`) runs the same points once, for its time.  GATE: A is faster than B.

Environment: N, PB, DEG, ROWS, ROUNDS (A/B rounds, default 3), DTYPE (f64 / f32), ORACLE (0: skip the CPU oracle)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import coordinatedescent_jl_amd as cd  # noqa: E402
from coordinatedescent_jl_amd.api import _lvocv_point, _vp  # noqa: E402

n, pb, deg = int(os.environ.get("N", 200_000)), int(os.environ.get("PB", 20)), int(os.environ.get("DEG", 1))
nrows, rounds = int(os.environ.get("ROWS", 100)), int(os.environ.get("ROUNDS", 3))
dtype = np.float32 if os.environ.get("DTYPE", "f64") == "f32" else np.float64
ep, hArr, lam0 = pb * (deg + 1), [0.05, 0.2], 0.3
opt = cd.CDOptions(maxIter=2000, optTol=1e-8, randomize=False, warmStart=True)
print(f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; n={n} p_base={pb} degree={deg} "
      f"{np.dtype(dtype).name} bandwidths={hArr} rows={nrows} rounds={rounds}", flush=True)

rng = np.random.default_rng(2025)
X = np.asfortranarray(rng.standard_normal((n, pb)).astype(dtype))
z = rng.random(n).astype(dtype)
s = min(3, pb)
y = ((np.sin(z[:, None].astype(np.float64) * rng.choice([2, 4, 6, 8], size=s)) * X[:, :s]).sum(axis=1)
     + 0.1 * rng.standard_normal(n)).astype(dtype)
rows = np.sort(rng.choice(n, size=nrows, replace=False))
y64 = y.astype(np.float64)

fA = cd.CDVaryingCoefficientLoss(y, X, z, deg)
fB = cd.CDWeightedLSLoss.__new__(cd.CDWeightedLSLoss)
fB._create(dtype, n, ep, 0, None, 0)
cd.check(fB._L.cdh_set_y(fB._h, _vp(np.ascontiguousarray(y))), fB._h)
eX = np.empty((n, ep), dtype=dtype, order="F")
eX[:, ::deg + 1] = X
z64 = z.astype(np.float64)
all_cols = np.arange(1, ep + 1, dtype=np.int64)


def setup_a(kernel, i):
    return fA.set_point_leave_out(kernel, i)


def setup_b(kernel, i):
    w = cd.evaluate(kernel, z64, float(z[i])).astype(dtype)
    w[i] = 0
    df = z - z[i]
    for l in range(1, deg + 1):
        np.multiply(eX[:, l - 1::deg + 1], df[:, None], out=eX[:, l::deg + 1])
    cd.check(fB._L.cdh_set_X_cols(fB._h, 0, ep, _vp(eX), n), fB._h)
    cd.check(fB._L.cdh_set_obs_weights(fB._h, _vp(w)), fB._h)
    sx = cd.stdX(fB, weighted=True)
    cd.check(fB._L.cdh_initialize(fB._h, ep, 0, None, None), fB._h)            # r = y: X_j'Wr is X_j'Wy
    fB._synced = None
    scores = np.zeros(ep)
    cd.check(fB._L.cdh_xt_r_cols(fB._h, ep, _vp(all_cols), _vp(scores)), fB._h)
    return sx, np.abs(scores)


def run(f, setup):
    beta, sq, t_setup = cd.SparseIterate(ep), [], 0.0
    solves = 0
    t0 = time.perf_counter()
    for h in hArr:
        kernel = cd.createKernel(cd.GaussianKernel, h)
        for i in rows:
            ts = time.perf_counter()
            sx, scores = setup(kernel, int(i))
            t_setup += time.perf_counter() - ts
            rec = _lvocv_point(f, beta, int(i), sx, scores, lam0, opt, y64[i], pb, deg)
            assert all(st["converged"] for st in rec["solves"])
            solves += rec["sigma_iters"]
            sq.append(rec["sq_err"])
    total = time.perf_counter() - t0
    return total, np.array(sq), {"point_setup_s": t_setup, "screening_solves_refit_s": total - t_setup, "solves": solves}


def spread(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1]}


runs = {"A": [], "B": []}
for r in range(rounds + 1):                                       # round 0 warms both routes up and is not counted
    for name, f, setup in (("A", fA, setup_a), ("B", fB, setup_b)):
        t, sq, extra = run(f, setup)
        print(f"  round {r}{' (warm-up)' if r == 0 else ''} route {name}: {t:.3f} s {json.dumps(extra)}", flush=True)
        if r:
            runs[name].append((t, sq, extra))
tA, tB = spread([t for t, _, _ in runs["A"]]), spread([t for t, _, _ in runs["B"]])
dsq = float(np.max(np.abs(runs["A"][-1][1] - runs["B"][-1][1])))
res = {"points": len(hArr) * nrows, "device_setup_route_s": tA, "host_setup_route_s": tB, "speedup": tB["median"] / tA["median"],
       "A_point_setup_s": spread([e["point_setup_s"] for _, _, e in runs["A"]]),
       "A_rest_s": spread([e["screening_solves_refit_s"] for _, _, e in runs["A"]]),
       "B_point_setup_s": spread([e["point_setup_s"] for _, _, e in runs["B"]]),
       "B_rest_s": spread([e["screening_solves_refit_s"] for _, _, e in runs["B"]]),
       "solves": runs["A"][-1][2]["solves"], "max_abs_diff_of_squared_errors_between_routes": dsq}
if os.environ.get("ORACLE", "1") != "0":
    import oracle as O
    from _vc_cv_numpy import oracle_lvocv
    t0 = time.perf_counter()
    _, pts = oracle_lvocv(O, X, z, y, deg, "gaussian", hArr, lam0, rows=[int(i) for i in rows], maxIter=2000, optTol=1e-8,
                          randomize=False)
    res["cpu_oracle_s"] = time.perf_counter() - t0
    want = np.array([(p["yhat"] - y64[p["row"]]) ** 2 for p in pts])
    res["max_abs_diff_of_squared_errors_to_cpu_oracle"] = float(np.max(np.abs(runs["A"][-1][1] - want)))
print(json.dumps(res), flush=True)
assert tA["max"] < tB["min"], "GATE: the device point setup must make the loop faster than host setup + uploads"
print("GATE met: the device route is faster", flush=True)
