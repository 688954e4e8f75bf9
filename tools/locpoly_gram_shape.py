#!/usr/bin/env python3
"""locpoly over a grid of 20 points at n = 1 000 000, p in {10, 50}, degree 1 and 2, fp64, Gaussian kernel, two routes on the
same handle, interleaved:

 A. cdh_vc_gram (k_vc_moments, streamed, on one point: one pass over the p base columns, z and y) + the host solve of the scaled
    normal equations;
 B. the best route the C ABI offered before it: cdh_vc_set_point (writes the p Q expanded columns) + cdh_initialize (r = y) +
    cdh_gram_weighted over all p (Q + 1) columns (<= 64 per launch, pairs of 32-column groups beyond) + the same host solve;

and a device-to-device copy of the bytes route A's kernel reads, n sz (p + 2), as the yardstick of a stream (a copy moves them
twice: read and write).  Times are host clocks around calls that end in a stream synchronise.  Writes the report to OUT
(default profiles/locpoly_gram.txt).  Environment: N, POINTS, ROUNDS, OUT."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import coordinatedescent_jl_amd as cd  # noqa: E402
from coordinatedescent_jl_amd.api import _solve_scaled, _vp  # noqa: E402

n, npoints, rounds = int(os.environ.get("N", 1_000_000)), int(os.environ.get("POINTS", 20)), int(os.environ.get("ROUNDS", 3))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "locpoly_gram.txt"))
kernel, zgrid = cd.GaussianKernel(0.1), np.linspace(0.05, 0.95, npoints)
lines = [f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; n={n} points={npoints} rounds={rounds} float64"]
print(lines[0], flush=True)


def spread(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1]}


def route_a(f):
    t0 = time.perf_counter()
    out = cd.locpoly(f, None, None, zgrid, None, kernel)
    return time.perf_counter() - t0, out


def route_b(f):
    ep = f.p
    idx1 = np.arange(1, ep + 1, dtype=np.int64)
    G, c, out = np.zeros((ep, ep)), np.zeros(ep), np.zeros((ep, npoints))
    t0 = time.perf_counter()
    for i, z0 in enumerate(zgrid):
        f.set_point(kernel, z0)
        cd.check(f._L.cdh_initialize(f._h, ep, 0, None, None), f._h)           # beta = 0: r = y, so X'Wr is X'Wy
        cd.check(f._L.cdh_gram_weighted(f._h, ep, _vp(idx1), _vp(G), _vp(c), None), f._h)
        out[:, i] = _solve_scaled(G, c)
    return time.perf_counter() - t0, out


for p in (10, 50):
    rng = np.random.default_rng(p)
    X = np.empty((n, p), order="F")
    for j in range(p):
        X[:, j] = rng.standard_normal(n)
    z = rng.random(n)
    y = (np.sin(4 * z) * X[:, 0] + np.cos(6 * z) * X[:, 1] + 0.1 * rng.standard_normal(n))
    for deg in (1, 2):
        f = cd.CDVaryingCoefficientLoss(y, X, z, deg)
        route_a(f), route_b(f)                                                 # warm-up of both
        ta, tb, diff = [], [], 0.0
        for _ in range(rounds):
            a, oa = route_a(f)
            b, ob = route_b(f)
            ta.append(a), tb.append(b)
            diff = max(diff, float(np.max(np.abs(oa - ob)) / np.max(np.abs(oa))))
        f.close()
        read_bytes = n * 8 * (p + 2)
        src = torch.empty(read_bytes // 8, dtype=torch.float64, device="cuda").normal_()
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)
        torch.cuda.synchronize()
        cp = []
        for _ in range(10):
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            cp.append(time.perf_counter() - t0)
        del src, dst
        sa, sb, sc = spread(ta), spread(tb), spread(cp)
        res = {"p": p, "degree": deg, "vc_gram_route_s_per_grid": sa, "set_point_gram_weighted_route_s_per_grid": sb,
               "ratio_B_over_A_medians": sb["median"] / sa["median"], "A_ms_per_point": 1e3 * sa["median"] / npoints,
               "kernel_read_bytes_per_point": read_bytes, "d2d_copy_of_those_bytes_ms": 1e3 * sc["median"],
               "A_GBps_on_read_bytes_whole_call": read_bytes / (sa["median"] / npoints) / 1e9,
               "max_rel_diff_of_coefficients": diff}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
