#!/usr/bin/env python3
"""The concordance index on the device against its yardsticks.  Prints ONE JSON line.

Run without arguments it is a driver: each measurement below runs in a child process of its own under `timeout -k 10`, in order,
and nothing runs after a child that failed or timed out (its status is in the line).  With --step NAME it is that child.

  conc_random, conc_sorted   on an fp64 handle of N rows (default 2 000 000) and one column, with an offset, STRATA strata
      (default 100; ids uniform over the rows), observation weights uniform in [0.25, 4] normalised to sum to n, times rounded
      to DECIMALS decimals (default 4), three rows in ten censored, 5 folds; rows in random order, or pre-sorted by (stratum,
      time).  Timed, interleaved call by call, REPS calls each per round, ROUNDS rounds (reported: the rounds' minima, their
      minimum and spread; host clocks around calls that end in a stream synchronise):
        conc_all           (a) cdh_glm_cox_concordance(k = -1)
        conc_fold          (a) cdh_glm_cox_concordance(k = 2): the held-out rows of one fold of five
        step_apply0        (b) cdh_glm_cox_irls(k = -1, apply = 0): the handle's read-only step
        copy_bytes         (c) a device-to-device copy of the bytes the concordance kernels move, counted per row of the N
                           planned positions (n rounded up to tiles of 1024) -- gathers counted as their useful bytes, the
                           binary searches' probes and the fringes' reads (which neighbouring lanes share) not at all:
                             k_conc_tile    68: order 4, y 8, r 8, offset 8, weight 8 in; key0, v0 and the sorted tile's keys
                                            and prefix sums out, 32 (the fold id, 1, with k >= 0)
                             k_conc_fringe  48: v0 8, qa 4, qb 4, key0 8 in; L, E, G out, 24
                             k_conc_level   112 a level: v0, qa, qb, key0 24 and L, E, G in and out 48 for the queries; key
                                            and prefix sum in 16, the sibling's prefix sum gathered 8, key and prefix sum
                                            scattered out 16 for the merge (the last level merges nothing: 72)
                             k_conc_rows    40: v0, qa, qb 16, L, E, G 24 in
                           with levels = top - 10 of them (the tile's to the one below the top; the one run of level top is
                           never taken), top = ceil(log2 N): 11 at n = 2 000 000, 1 348 bytes a row; the
                           copy reads and writes half of them
      and, once, (d) the host-composed alternative: y and r downloaded (cdh_get_y, cdh_get_residual), then the twin's
      level-by-level form in numpy (tests/_cox_concordance_numpy.levels_vectorised) with NOTHING cached -- the sort included.
      The line carries (a)/(b), (a)/(c), (d)/(a) and the differences of the device's three numbers from the host's, relative
      to their total.
  cv   cvCoxLassoPath on a loss of N2 rows and P2 columns (default 2 000 000 x 1000), 5 folds x M2 = 30 lambdas from 0.9 to
      0.05 of lambda_max, full_path=False, under measure="deviance" and under measure="C", once each after a warm-up on the
      first two lambdas: the wall times, their ratio, and the two selections.

Environment: N, REPS, ROUNDS, STRATA, DECIMALS, N2, P2, M2, STEP_TIMEOUT, CV_TIMEOUT, STEPS (a comma-separated subset of the
steps), OUT (a file that receives the line too)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
env = lambda k, d: int(os.environ.get(k, d))  # noqa: E731
STEPS = tuple(os.environ.get("STEPS", "conc_random,conc_sorted,cv").split(","))


def driver():
    res, ok = {}, True
    for name in STEPS:
        if not ok:
            res[name] = {"skipped": "an earlier step failed"}
            continue
        limit = env("CV_TIMEOUT", 420) if name == "cv" else env("STEP_TIMEOUT", 240)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        last = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not last:
            res[name] = {"failed": p.returncode, "stderr_tail": p.stderr[-400:]}
            ok = False
        else:
            res[name] = json.loads(last[-1])
        print("cox_concordance_timing: %s %s" % (name, "done" if ok else "failed"), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT"):
        os.makedirs(os.path.dirname(os.path.abspath(os.environ["OUT"])), exist_ok=True)
        with open(os.environ["OUT"], "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if "--step" not in sys.argv:
    sys.exit(driver())

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coordinatedescent_jl_amd as cd  # noqa: E402
import _cox_concordance_numpy as CC  # noqa: E402

step = sys.argv[sys.argv.index("--step") + 1]
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
PD = C.POINTER(C.c_double)
WMIN, ETA_MAX = 1e-5, 50.0
STRATA, DECIMALS = env("STRATA", 100), env("DECIMALS", 4)
TILE, STEP_BYTES = 1024, 228      # (the read-only strata step: the applied step's 252 less its three scattered stores)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def survival(f, seed, presorted):
    """The data of tools/cox_post_timing.py, set on the handle; -> (t, status, off, g, v)."""
    n = f.n
    rng = np.random.default_rng(seed)
    sig = f.y
    off = rng.uniform(-0.5, 0.5, n)
    t = np.round(rng.exponential(1.0, n) / np.exp(0.5 * sig / np.std(sig) + off), DECIMALS)
    status = (rng.random(n) >= 0.3).astype(np.float64)
    g = rng.integers(0, STRATA, n).astype(np.int32)
    v = rng.uniform(0.25, 4.0, n)
    v = v * n / v.sum()
    if presorted:
        o = np.lexsort((t, g))
        t, g = np.ascontiguousarray(t[o]), np.ascontiguousarray(g[o])
    cd.check(f._L.cdh_glm_set_survival_strata(f._h, vp(t), vp(status), vp(off), vp(g), vp(v)), f._h)
    f._weighted = True          # the loss came from generate() and got its weights through the C setter: tell the front end, whose
                                # cvCoxLassoPath reads the flag to weight the folds (tools/cox_timing.py does the same)
    return t, status, off, g, v


def conc_bytes(n):
    N = -(-n // TILE) * TILE
    top = max(10, (N - 1).bit_length())
    levels = top - 10
    return N, levels, 68 + 48 + (112 * (levels - 1) + 72 if levels else 0) + 40


def measure(presorted):
    n, reps, rounds = env("N", 2_000_000), env("REPS", 5), env("ROUNDS", 3)
    f, _ = cd.CDCoxLoss.generate(n, 1, seed=7, s=1, noise=1.0)
    t, status, off, g, v = survival(f, 7, presorted)
    L, h = f._L, f._h
    x = cd.SparseIterate(1)
    x[1] = 0.5
    cd.initialize_(f, x)
    ids = (np.random.default_rng(8).permutation(n) % 5).astype(np.int32)
    f.set_folds(ids, 5)
    out5, out_all, out_fold = np.zeros(5), np.zeros(4), np.zeros(4)
    N, levels, bytes_a_row = conc_bytes(n)

    def step0():
        cd.check(L.cdh_glm_cox_irls(h, -1, 0, WMIN, ETA_MAX, out5.ctypes.data_as(PD)), h)

    def conc_all():
        cd.check(L.cdh_glm_cox_concordance(h, -1, out_all.ctypes.data_as(PD)), h)

    def conc_fold():
        cd.check(L.cdh_glm_cox_concordance(h, 2, out_fold.ctypes.data_as(PD)), h)

    src = torch.randn(bytes_a_row // 2 * N // 8, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    first_call = timed(conc_all)[0]                              # the order is derived and uploaded here
    names = ("conc_all", "conc_fold", "step_apply0", "copy_bytes")
    fns = (conc_all, conc_fold, step0, copy)
    for fn in fns:
        fn()
    per = {k: [] for k in names}
    for _ in range(rounds):
        ts = [[] for _ in fns]
        for _ in range(reps):
            for tt, fn in zip(ts, fns):
                tt.append(timed(fn)[0])
        for k, tt in zip(names, ts):
            per[k].append(min(tt))

    def host():
        eta = (f.y - f.r) + off
        return CC.levels_vectorised(t, status, eta, strata=g, weights=v)

    sec, want = timed(host)
    sec_fold, want_fold = timed(lambda: CC.levels_vectorised(t, status, (f.y - f.r) + off, strata=g, weights=v, subset=ids == 2))
    res = {"n": n, "positions": N, "presorted": presorted, "strata": STRATA, "decimals": DECIMALS, "levels": levels,
           "bytes_a_row": {"concordance": bytes_a_row, "step_apply0": STEP_BYTES}, "first_call_ms": 1e3 * first_call}
    for k, vv in per.items():
        res[k] = {"round_minima_ms": [1e3 * a for a in vv], "min_ms": 1e3 * min(vv), "spread_ms": 1e3 * (max(vv) - min(vv))}
    best = {k: min(vv) for k, vv in per.items()}
    res["conc_all_over_step"] = best["conc_all"] / best["step_apply0"]
    res["conc_fold_over_step"] = best["conc_fold"] / best["step_apply0"]
    res["conc_all_over_copy"] = best["conc_all"] / best["copy_bytes"]
    res["conc_fold_over_copy"] = best["conc_fold"] / best["copy_bytes"]
    res["host_composed_ms"] = 1e3 * sec
    res["host_composed_fold_ms"] = 1e3 * sec_fold
    res["host_composed_over_conc_all"] = sec / best["conc_all"]
    res["host_composed_over_conc_fold"] = sec_fold / best["conc_fold"]
    res["counts_all"] = [float(a) for a in out_all]
    res["C_all"], res["C_fold"] = CC.cindex(*out_all[:3]), CC.cindex(*out_fold[:3])
    tot, tot_fold = float(sum(want)), float(sum(want_fold))
    res["max_rel_device_minus_host"] = max(abs(float(out_all[i]) - float(want[i])) for i in range(3)) / tot
    res["max_rel_device_minus_host_fold"] = max(abs(float(out_fold[i]) - float(want_fold[i])) for i in range(3)) / tot_fold
    print(json.dumps(res), flush=True)


def measure_cv():
    n, p, m = env("N2", 2_000_000), env("P2", 1000), env("M2", 30)
    f, _ = cd.CDCoxLoss.generate(n, p, seed=11, s=10, noise=1.0)
    survival(f, 11, False)
    lmax = cd.coxLambdaMax(f)
    lam = lmax * np.geomspace(0.9, 0.05, m)
    ids = np.random.default_rng(12).permutation(n) % 5
    kw = dict(K=5, folds=ids, options=cd.CDOptions(maxIter=2000, optTol=1e-7, randomize=False), irls=cd.IRLSOptions(maxIter=100),
              standardizeX=False, full_path=False)
    for measure_ in ("deviance", "C"):
        cd.cvCoxLassoPath(f, None, lam[:2], measure=measure_, **kw)
    sec_d, dev = timed(lambda: cd.cvCoxLassoPath(f, None, lam, measure="deviance", **kw))
    sec_c, con = timed(lambda: cd.cvCoxLassoPath(f, None, lam, measure="C", **kw))
    res = {"n": n, "p": p, "lambdas": m, "folds": 5, "strata": STRATA, "cv_deviance_s": sec_d, "cv_C_s": sec_c, "C_over_deviance": sec_c / sec_d,
           "rounds": int(con.rounds.sum()), "same_fold_deviance": bool(np.array_equal(dev.fold_deviance, con.fold_deviance)),
           "index_min_deviance": dev.index_min, "index_min_C": con.index_min, "index_1se_C": con.index_1se,
           "cvm_C": [float(a) for a in con.cvm]}
    print(json.dumps(res), flush=True)


if step == "cv":
    measure_cv()
else:
    measure(step == "conc_sorted")
