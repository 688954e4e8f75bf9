#!/usr/bin/env python3
"""Neighbourhood selection of a p-variable graph as ONE batch of covariance-form problems (default p = m = 1000): A is the
sample correlation of an n x p AR(1) design (n = 2000, rho = 0.5), problem j has b_j = -A_j and omega_jj = inf (variable j is
regressed on the others), one lambda for all.  Three routes to the same m solutions, warm-started from zero, ordered sweeps:

 A. cd.CDQuadraticLoss(A, B): all m problems in one launch (k_quad_solve, one workgroup per problem);
 B. the CPU oracle (oracle.CDQuadraticLoss) on one core, problem after problem;
 C. the best route the library had before: one CDLeastSquaresLoss handle on the standardised design, cdh_set_y per column,
    the one-launch solve (k_solve_small on the handle's Gram matrix) for each column.

Prints the three times (A also as the library call alone, without the Python mirror's per-problem fetch of the iterates),
the non-zeros per column and the largest difference between the routes' beta; writes the same lines to OUT
(default profiles/quad_batch.txt).  Not gated: whichever of A and C is faster, the file says so.

Environment: P, M (<= P), N, RHO, LAM, ROUNDS (default 3), ORACLE (0: skip route B), OUT."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import coordinatedescent_jl_amd as cd  # noqa: E402
from coordinatedescent_jl_amd.api import _vp  # noqa: E402

p, n = int(os.environ.get("P", 1000)), int(os.environ.get("N", 2000))
m, rho, lam = int(os.environ.get("M", p)), float(os.environ.get("RHO", 0.5)), float(os.environ.get("LAM", 0.035))
rounds, out_path = int(os.environ.get("ROUNDS", 3)), os.environ.get("OUT", os.path.join(ROOT, "profiles", "quad_batch.txt"))
opt = cd.CDOptions(maxIter=2000, optTol=1e-8, randomize=False, warmStart=True)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say(f"device: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}; neighbourhood selection p={p} m={m} n={n} AR(1) rho={rho} "
    f"lambda={lam} optTol={opt.optTol} ordered, warm from zero, rounds={rounds}")
rng = np.random.default_rng(2026)
E = rng.standard_normal((n, p))
X = np.empty((n, p), order="F")
X[:, 0] = E[:, 0]
for j in range(1, p):
    X[:, j] = rho * X[:, j - 1] + np.sqrt(1 - rho * rho) * E[:, j]
X -= X.mean(axis=0)
X /= np.sqrt((X * X).sum(axis=0) / n)
A = X.T @ X / n
A = (A + A.T) / 2
B = np.asfortranarray(-A[:, :m])
omega = np.ones((p, m), order="F")
omega[np.arange(m), np.arange(m)] = np.inf

# ---- A: the batch ------------------------------------------------------------------------------------------------------
f = cd.CDQuadraticLoss(A, B)
gs = [cd.ProxL1(lam, omega[:, j]) for j in range(m)]
tA, tA_call = [], []
for r in range(rounds + 1):
    f.set_b(B)
    xs = [cd.SparseIterate(p) for _ in range(m)]
    t0 = time.perf_counter()
    cd.coordinateDescent_(xs, f, gs, opt)
    t1 = time.perf_counter()
    o, st = opt._c(), (cd.cdh_stats * m)()        # the library call alone, on the same problems from the same start
    f.set_b(B)
    f._set_penalties(gs)
    t2 = time.perf_counter()
    f._q(f._L.cdh_quad_coordinate_descent(f._h, C.byref(o), st))
    t3 = time.perf_counter()
    if r:                                         # (round 0 warms up)
        tA.append(t1 - t0)
        tA_call.append(t3 - t2)
betaA = np.stack([x.dense() for x in xs], axis=1)
nnz = (betaA != 0).sum(axis=0)
passes = [s["passes"] for s in f.last_stats]
say(f"non-zeros per column: min {nnz.min()} median {int(np.median(nnz))} max {nnz.max()}; passes per problem: min {min(passes)} "
    f"max {max(passes)}; all converged: {all(s['converged'] for s in f.last_stats)}")
say(f"A  batch, one launch:            {statistics.median(tA_call) * 1e3:9.2f} ms the library call, {statistics.median(tA) * 1e3:9.2f} ms "
    f"with penalties, iterates up and back through the Python mirror")
f.close()

# ---- C: the least-squares handle, column after column ------------------------------------------------------------------------
os.environ["CDH_SMALL_PATH"] = "1"
fl = cd.CDLeastSquaresLoss(X[:, 0].copy(), X)
tC = []
betaC = np.zeros((p, m))
for r in range(rounds + 1):
    t0 = time.perf_counter()
    for j in range(m):
        y = np.ascontiguousarray(X[:, j])
        cd.check(fl._L.cdh_set_y(fl._h, _vp(y)), fl._h)
        x = cd.SparseIterate(p)
        cd.coordinateDescent_(x, fl, gs[j], opt)
        if r == rounds:
            betaC[:, j] = x.dense()
    if r:
        tC.append(time.perf_counter() - t0)
say(f"C  cdh_set_y + one-launch solve per column: {statistics.median(tC) * 1e3:9.2f} ms ({fl.onchip_stats()})")
fl.close()
say(f"max |beta_A - beta_C| = {np.abs(betaA - betaC).max():.3e}")

# ---- B: the oracle on one core -----------------------------------------------------------------------------------------------
if os.environ.get("ORACLE", "1") != "0":
    import oracle as O  # noqa: E402
    oo = O.CDOptions(maxIter=opt.maxIter, optTol=opt.optTol, randomize=False, warmStart=True)
    betaB = np.zeros((p, m))
    t0 = time.perf_counter()
    for j in range(m):
        fo, xo = O.CDQuadraticLoss(A, np.ascontiguousarray(B[:, j])), O.SparseIterate(p)
        O.coordinateDescent_(xo, fo, O.ProxL1(lam, omega[:, j]), oo)
        betaB[:, j] = xo.dense()
    tB = time.perf_counter() - t0
    say(f"B  CPU oracle, one core:         {tB * 1e3:9.2f} ms")
    say(f"max |beta_A - beta_B| = {np.abs(betaA - betaB).max():.3e}")
best = statistics.median(tA_call)
say(f"A against C: {statistics.median(tC) / best:.2f}x (the library call), {statistics.median(tC) / statistics.median(tA):.2f}x (through the mirror)")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
