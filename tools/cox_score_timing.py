#!/usr/bin/env python3
"""cdh_glm_cox_score on the device against its yardsticks.  Prints ONE JSON line.

Run without arguments it is a driver: each measurement below runs in a child process of its own under `timeout -k 10`, in order,
and nothing runs after a child that failed or timed out (its status is in the line).  With --step NAME it is that child.

  score_random, score_sorted   on an fp64 handle of N rows (default 2 000 000) and P columns (default 1000), with an offset,
      STRATA strata (default 100), observation weights uniform in [0.25, 4] normalised to sum to n, times rounded to DECIMALS
      decimals, three rows in ten censored; rows in random order, or pre-sorted by (stratum, time); an iterate on eight columns.
      For m in MS (default 1, 8, 64) columns spread over the design, timed, interleaved call by call, REPS calls each per round,
      ROUNDS rounds (reported: the rounds' minima, their minimum and spread; host clocks around calls that end in a stream
      synchronise -- a call INCLUDES the download of its answer, n m doubles per residual output):
        sch, score, info     (a) the call with that output alone
        all                  (a) the call with the three outputs
        step_apply0          (b) cdh_glm_cox_irls(k = -1, apply = 0): the handle's read-only step, which every call runs first
        copy                 (c) a device-to-device copy of the bytes the chain moves by the estimate of DESIGN.md 5k (38), written
                             before measuring: per row 228 (the step) + 100 (k_score_prep); per (row, column) 36 (gather) + 20 + 20
                             (the scans) + 44 (mean), and 84 more when a residual is asked for (rows); with the matrix 88 per
                             (row, pair tile).  Timed on a buffer of at most COPY_GIB GiB (default 2) and scaled by the bytes.
      and, once per m in HOST_MS (default 1, 8), (d) the host-composed alternative: y and r downloaded (cdh_get_y,
      cdh_get_residual), the m columns (cdh_get_X_cols), and the twin's scan half in float64 (tests/_cox_score_numpy.scan:
      cumulative sums per stratum).  The line carries (a)/(b), (a)/(c), (d)/(a) and the largest differences of the device's
      answers from the host's, relative to the largest entry.

Environment: N, P, REPS, ROUNDS, STRATA, DECIMALS, MS, HOST_MS, COPY_GIB, STEP_TIMEOUT, STEPS (a comma-separated subset of the
steps), OUT (the file that receives the line too; default profiles/cox_score_timing.txt)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
env = lambda k, d: int(os.environ.get(k, d))  # noqa: E731
STEPS = tuple(os.environ.get("STEPS", "score_random,score_sorted").split(","))


def driver():
    res, ok = {}, True
    for name in STEPS:
        if not ok:
            res[name] = {"skipped": "an earlier step failed"}
            continue
        p = subprocess.run(["timeout", "-k", "10", str(env("STEP_TIMEOUT", 420)), sys.executable, os.path.abspath(__file__),
                            "--step", name], capture_output=True, text=True)
        last = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not last:
            res[name] = {"failed": p.returncode, "stderr_tail": p.stderr[-400:]}
            ok = False
        else:
            res[name] = json.loads(last[-1])
        print("cox_score_timing: %s %s" % (name, "done" if ok else "failed"), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "cox_score_timing.txt"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    return 0 if ok else 1


if "--step" not in sys.argv:
    sys.exit(driver())

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coordinatedescent_jl_amd as cd  # noqa: E402
import _cox_score_numpy as CSN  # noqa: E402

step = sys.argv[sys.argv.index("--step") + 1]
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
PD = C.POINTER(C.c_double)
WMIN, ETA_MAX = 1e-5, 50.0
STRATA, DECIMALS = env("STRATA", 100), env("DECIMALS", 4)
MS = tuple(int(a) for a in os.environ.get("MS", "1,8,64").split(","))
HOST_MS = tuple(int(a) for a in os.environ.get("HOST_MS", "1,8").split(","))
PAIR = 4


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def chain_bytes(m, residual, info):
    """bytes a row by the estimate of DESIGN.md 5k (38)"""
    ct = -(-m // PAIR)
    return 228 + 100 + m * (36 + 20 + 20 + 44 + (84 if residual else 0)) + (88 * (ct * (ct + 1) // 2) if info else 0)


def measure(presorted):
    n, p, reps, rounds = env("N", 2_000_000), env("P", 1000), env("REPS", 3), env("ROUNDS", 3)
    f, _ = cd.CDCoxLoss.generate(n, p, seed=7, s=8, noise=1.0)
    rng = np.random.default_rng(7)
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
    L, h = f._L, f._h
    x = cd.SparseIterate(p)
    for j in range(8):
        x[1 + j * (p // 8)] = 0.1 * (-1) ** j
    cd.initialize_(f, x)
    out5 = np.zeros(5)
    lists = {m: np.ascontiguousarray(1 + (np.arange(m) * (p // m) + 3) % p, dtype=np.int64) for m in MS}
    bufs = {m: (np.zeros((n, m), order="F"), np.zeros((n, m), order="F"), np.zeros((m, m)), np.zeros(m)) for m in MS}

    def step0():
        cd.check(L.cdh_glm_cox_irls(h, -1, 0, WMIN, ETA_MAX, out5.ctypes.data_as(PD)), h)

    def call(m, what):
        sch, sc, info, mu = bufs[m]
        want = {"sch": (sch, None, None), "score": (None, sc, None), "info": (None, None, info), "all": (sch, sc, info)}[what]
        return lambda: cd.check(L.cdh_glm_cox_score(h, ETA_MAX, m, vp(lists[m]), None, vp(mu), *[vp(a) for a in want]), h)

    chunk = min(env("COPY_GIB", 2) << 30, chain_bytes(max(MS), True, True) * n // 2)
    src = torch.randn(chunk // 8, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    names = ["step_apply0", "copy"] + ["%s_m%d" % (w, m) for m in MS for w in ("sch", "score", "info", "all")]
    fns = [step0, copy] + [call(m, w) for m in MS for w in ("sch", "score", "info", "all")]
    first_call = timed(fns[-1])[0]                               # the scratch for the largest m is allocated here
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
    res = {"n": n, "p": p, "presorted": presorted, "strata": STRATA, "decimals": DECIMALS, "first_call_ms": 1e3 * first_call,
           "copy_chunk_bytes": 2 * chunk}
    for k, vv in per.items():
        res[k] = {"round_minima_ms": [1e3 * a for a in vv], "min_ms": 1e3 * min(vv), "spread_ms": 1e3 * (max(vv) - min(vv))}
    best = {k: min(vv) for k, vv in per.items()}
    for m in MS:
        for w in ("sch", "score", "info", "all"):
            k = "%s_m%d" % (w, m)
            b = chain_bytes(m, w != "info", w in ("info", "all"))
            copy_s = best["copy"] * b * n / (2 * chunk)
            res[k].update({"bytes_a_row": b, "copy_of_bytes_ms": 1e3 * copy_s, "over_step": best[k] / best["step_apply0"],
                           "over_copy": best[k] / copy_s})
    for m in HOST_MS:
        if m not in MS:
            continue
        cols = lists[m]

        def host():
            y, r = f.y, f.r
            X = np.zeros((n, m), order="F")
            for c, j in enumerate(cols):
                cd.check(L.cdh_get_X_cols(h, int(j) - 1, 1, vp(X[:, c]), n), h)
            return CSN.scan(X, y - r, off, t, status, ETA_MAX, strata=g, weights=v, centre=bufs[m][3], dtype=np.float64)

        call(m, "all")()
        sec, q = timed(host)
        sch, sc, info, _ = bufs[m]
        rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))  # noqa: E731
        res["host_m%d" % m] = {"host_composed_ms": 1e3 * sec, "over_all": sec / best["all_m%d" % m],
                               "max_rel_device_minus_host": {"sch": rel(sch, q["sch"]), "score": rel(sc, q["score"]),
                                                             "info": rel(info, q["info"])}}
    print(json.dumps(res), flush=True)


measure(step == "score_sorted")
