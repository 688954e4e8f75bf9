#!/usr/bin/env python3
"""The loadings pass of feasibleLasso_ against its yardstick, and the front end against the CPU restatement.

 1. cdh_loadings (k_col_loadings) against cdh_col_rms (k_col_dots) on ONE fp64 handle whose columns stream from HBM
    (default n = 1 000 000, p = 2000: 16 GB, generated on the device), r = y.  Both come from the library as built; cdh_col_rms
    streams the same bytes on the same grid, so it is the yardstick.  The two are interleaved call by call, REPS calls each
    per round, ROUNDS rounds; reported are each round's minimum, the minimum and the spread of those over the rounds, and
    the rate on the algorithmic bytes n sz p (1 + 1/8).  Times are host clocks around calls that end in a stream
    synchronise and a copy of p doubles.
 2. feasibleLasso_ (default n = 20 000, p = 500, the heteroscedastic recipe of tests/_feasible_oracle.py, :Screening) against
    the CPU restatement of lasso.jl:154-194 on the oracle: wall time of each, rounds, and the difference of the iterates.

Writes the report to OUT (default profiles/feasible_shape.txt).  Environment: N, P, REPS, ROUNDS, N2, P2, OUT."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coordinatedescent_jl_amd as cd  # noqa: E402
import oracle as O  # noqa: E402  (the checker)
import _feasible_oracle as FO  # noqa: E402

env = lambda k, d: int(os.environ.get(k, d))  # noqa: E731
n, p, reps, rounds = env("N", 1_000_000), env("P", 2000), env("REPS", 5), env("ROUNDS", 3)
n2, p2 = env("N2", 20_000), env("P2", 500)
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "feasible_shape.txt"))
lines = [f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; n={n} p={p} reps={reps} rounds={rounds} float64"]
print(lines[0], flush=True)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


# ---- 1. the pass against its yardstick ---------------------------------------------------------------------------------
f, _ = cd.CDLeastSquaresLoss.generate(n, p, seed=7, s=10, noise=1.0)
cd.check(f._L.cdh_initialize(f._h, p, 0, None, None), f._h)                   # beta = 0: r = y
cd.getLoadings(f), cd.stdX(f)                                                  # warm-up of both
per_round = {"cdh_loadings": [], "cdh_col_rms": []}
for _ in range(rounds):
    tl, tr = [], []
    for _ in range(reps):
        tl.append(timed(lambda: cd.getLoadings(f))[0])
        tr.append(timed(lambda: cd.stdX(f))[0])
    per_round["cdh_loadings"].append(min(tl))
    per_round["cdh_col_rms"].append(min(tr))
f.close()
bytes_alg = n * 8 * p * (1 + 1 / 8)
res = {"n": n, "p": p, "algorithmic_bytes": bytes_alg}
for k, v in per_round.items():
    res[k] = {"round_minima_ms": [1e3 * t for t in v], "min_ms": 1e3 * min(v), "spread_ms": 1e3 * (max(v) - min(v)),
              "TBps_on_algorithmic_bytes": bytes_alg / min(v) / 1e12}
res["loadings_over_col_rms"] = min(per_round["cdh_loadings"]) / min(per_round["cdh_col_rms"])
res["gap_ms"] = 1e3 * (min(per_round["cdh_loadings"]) - min(per_round["cdh_col_rms"]))
lines.append(json.dumps(res))
print(lines[-1], flush=True)

# ---- 2. the front end against the CPU restatement -------------------------------------------------------------------------
X, y, lam0 = FO.recipe(1, n2, p2)
fl = cd.CDLeastSquaresLoss(y, X)
o = cd.IterLassoOptions(optionsCD=cd.CDOptions(**FO.CD))
cd.feasibleLasso_(cd.SparseIterate(p2), fl, None, lam0, o)                     # warm-up
tg = []
for _ in range(rounds):
    x = cd.SparseIterate(p2)
    tg.append(timed(lambda: cd.feasibleLasso_(x, fl, None, lam0, o))[0])
fl.close()
tc, want = timed(lambda: FO.feasible_lasso(O.SparseIterate(p2), X, y, lam0))
res = {"n": n2, "p": p2, "init": "Screening", "lam0": lam0, "feasibleLasso_s": {"min": min(tg), "max": max(tg)},
       "cpu_restatement_s": tc, "cpu_over_gpu": tc / min(tg), "rounds_cpu": len(want.stats), "nnz": int(x.nnz),
       "max_abs_beta_diff": float(np.max(np.abs(x.dense() - want.x.dense())))}
lines.append(json.dumps(res))
print(lines[-1], flush=True)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
