#!/usr/bin/env python3
"""The Cox model's post-estimation exports against their yardsticks.  Prints ONE JSON line.

Run without arguments it is a driver: each measurement below runs in a child process of its own under `timeout -k 10`, in order,
and nothing runs after a child that failed or timed out (its status is in the line).  With --step NAME it is that child.

  post_random, post_sorted   on an fp64 handle of N rows (default 2 000 000) and one column, with an offset, STRATA strata
      (default 100; ids uniform over the rows), observation weights uniform in [0.25, 4] normalised to sum to n, times rounded
      to DECIMALS decimals (default 4: about half of the events tied), three rows in ten censored; rows in random order, or
      pre-sorted by (stratum, time).  EFRON=1 sets the handle to Efron ties.  Timed, interleaved call by call, REPS calls each per
      round, ROUNDS rounds (reported: the rounds' minima, their minimum and spread; host clocks around calls that end in a
      stream synchronise):
        step_apply0        cdh_glm_cox_irls(k = -1, apply = 0): the read-only step both exports run first
        residuals_one      cdh_glm_cox_residuals with the martingale residual alone (n doubles downloaded)
        residuals_three    ... with all three outputs (3 n doubles downloaded)
        baseline           cdh_glm_cox_baseline with capacity = the number of events (six columns of `table_rows` downloaded)
        baseline_count     cdh_glm_cox_baseline with every column NULL: the step and the table's launches, one double downloaded
        copy_rows, copy_table   a device-to-device copy of the bytes the ADDED kernels move: 68 a row for k_post_rows with one
                           output (order 4, last 4, y 8, r 8, status 8, offset 8, the scanned flag 8, slotpos 4 and hA 8
                           gathered, the scattered store 8), which the residuals' call moves ON TOP of the table's, and 108
                           a row for the table's five launches (mark 32, the scan of dv 20, flag 20, the scan of the flags 16,
                           scatter 20; the ~100 bytes per TABLE row are not counted); each copy reads and writes half of them
        download_one       a device-to-host copy of n doubles into pageable memory: what residuals_one cannot avoid
      and, once each, the same quantities composed on the host: y and r downloaded (cdh_get_y, cdh_get_residual), the twin's
      cumulative-sum form in numpy (tests/_cox_strata_numpy.scans, or tests/_cox_efron_numpy.scans with EFRON=1) with NOTHING
      cached -- the sort included, as a caller without this library's handle would have to -- then the martingale residuals and
      the table by np.add.reduceat over the tie groups.
      The line carries the ratios over the read-only step ("residuals_one_over_step", "baseline_over_step"), the ratios the
      byte counts predict (404 / 228 and 336 / 228 for the strata chain), and the largest differences of the
      device's martingale residuals and cumhaz column from the host's.

Environment: N, REPS, ROUNDS, STRATA, DECIMALS, EFRON, STEP_TIMEOUT, OUT (a file that receives the line too)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
env = lambda k, d: int(os.environ.get(k, d))  # noqa: E731
STEPS = ("post_random", "post_sorted")


def driver():
    res, ok = {}, True
    for name in STEPS:
        if not ok:
            res[name] = {"skipped": "an earlier step failed"}
            continue
        p = subprocess.run(["timeout", "-k", "10", str(env("STEP_TIMEOUT", 240)), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        last = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not last:
            res[name] = {"failed": p.returncode, "stderr_tail": p.stderr[-400:]}
            ok = False
        else:
            res[name] = json.loads(last[-1])
        print("cox_post_timing: %s %s" % (name, "done" if ok else "failed"), file=sys.stderr, flush=True)
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
import _cox_efron_numpy as CE  # noqa: E402
import _cox_numpy as CX  # noqa: E402
import _cox_strata_numpy as CS  # noqa: E402

step = sys.argv[sys.argv.index("--step") + 1]
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
PD = C.POINTER(C.c_double)
WMIN, ETA_MAX = 1e-5, 50.0
STRATA, DECIMALS, EFRON = env("STRATA", 100), env("DECIMALS", 4), env("EFRON", 0)
STEP_BYTES, ROWS_BYTES, TABLE_BYTES = 228, 68, 108


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def host_composed(f, t, status, off, g, v):
    """-> (seconds, martingale residuals, the table's cumhaz column), from the handle's y and r and nothing cached."""
    t0 = time.perf_counter()
    eta_lin = f.y - f.r
    ec, e, _ = CX.eta_of(eta_lin, off, ETA_MAX)
    ev, dv = v * e, v * status
    order, first, last, sfirst, slast = CS.groups(t, g)
    if EFRON:
        q, _ = CE.scans(ev, dv, t, g)
        A = np.empty(len(t))
        A[order] = q["A"]
        with np.errstate(divide="ignore", invalid="ignore"):
            h = np.where(q["ok"], q["mm"] / q["den"], 0.0)
        cum = CE._seg_cumsum(h, sfirst, slast)
    else:
        _, A, _ = CS.scans(ev, dv, t, g)
        cum = np.empty(len(t))
        cum[:] = A[order]
    M = status - e * A
    heads = np.nonzero(first == np.arange(len(t)))[0]
    nev = np.add.reduceat(dv[order], heads)
    cumhaz = cum[last[heads]][nev > 0]
    return time.perf_counter() - t0, M, cumhaz


def measure(presorted):
    n, reps, rounds = env("N", 2_000_000), env("REPS", 5), env("ROUNDS", 3)
    f, _ = cd.CDCoxLoss.generate(n, 1, seed=7, s=1, noise=1.0)
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
    L, h = f._L, f._h
    cd.check(L.cdh_glm_set_survival_strata(h, vp(t), vp(status), vp(off), vp(g), vp(v)), h)
    f._weighted = True
    if EFRON:
        cd.check(L.cdh_glm_set_cox_ties(h, 1), h)
    x = cd.SparseIterate(1)
    x[1] = 0.5
    cd.initialize_(f, x)
    events = int(status.sum())
    out5, M, three = np.zeros(5), np.zeros(n), [np.zeros(n) for _ in range(3)]
    stratum, cols, count = np.zeros(events, dtype=np.int32), [np.zeros(events) for _ in range(5)], C.c_int64()

    def step0():
        cd.check(L.cdh_glm_cox_irls(h, -1, 0, WMIN, ETA_MAX, out5.ctypes.data_as(PD)), h)

    def res_one():
        cd.check(L.cdh_glm_cox_residuals(h, ETA_MAX, None, vp(M), None), h)

    def res_three():
        cd.check(L.cdh_glm_cox_residuals(h, ETA_MAX, *[vp(a) for a in three]), h)

    def baseline():
        cd.check(L.cdh_glm_cox_baseline(h, ETA_MAX, events, vp(stratum), *[vp(c) for c in cols], C.byref(count)), h)

    def copier(bytes_a_row):
        src = torch.randn(bytes_a_row // 2 * n // 8, dtype=torch.float64, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()
        return copy

    dev = torch.randn(n, dtype=torch.float64, device="cuda")
    host = np.zeros(n)
    host_t = torch.from_numpy(host)

    def download():
        host_t.copy_(dev)
        torch.cuda.synchronize()

    def baseline_count():
        cd.check(L.cdh_glm_cox_baseline(h, ETA_MAX, events, None, None, None, None, None, None, C.byref(count)), h)

    names = ("step_apply0", "residuals_one", "residuals_three", "baseline", "baseline_count", "copy_rows", "copy_table", "download_one")
    fns = (step0, res_one, res_three, baseline, baseline_count, copier(ROWS_BYTES), copier(TABLE_BYTES), download)
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
    sec, M_host, cum_host = host_composed(f, t, status, off, g, v)
    m = count.value
    res = {"n": n, "presorted": presorted, "strata": STRATA, "efron": EFRON, "decimals": DECIMALS, "events": events, "table_rows": m,
           "bytes_a_row": {"step_apply0": STEP_BYTES, "rows_added": ROWS_BYTES, "table_added": TABLE_BYTES}}
    for k, vv in per.items():
        res[k] = {"round_minima_ms": [1e3 * a for a in vv], "min_ms": 1e3 * min(vv), "spread_ms": 1e3 * (max(vv) - min(vv))}
    best = {k: min(vv) for k, vv in per.items()}
    res["residuals_one_over_step"] = best["residuals_one"] / best["step_apply0"]
    res["residuals_one_less_download_over_step"] = (best["residuals_one"] - best["download_one"]) / best["step_apply0"]
    res["baseline_over_step"] = best["baseline"] / best["step_apply0"]
    res["predicted_from_bytes"] = {"residuals_one_over_step": (STEP_BYTES + TABLE_BYTES + ROWS_BYTES) / STEP_BYTES,
                                   "baseline_over_step": (STEP_BYTES + TABLE_BYTES) / STEP_BYTES}
    # the added launches alone: the table's from the call that downloads only the count, the rows' kernel from what the
    # residuals' call takes beyond that call and its one download
    res["table_launches_ms"] = 1e3 * (best["baseline_count"] - best["step_apply0"])
    res["rows_launch_ms"] = 1e3 * (best["residuals_one"] - best["download_one"] - best["baseline_count"])
    res["table_launches_over_copy"] = (best["baseline_count"] - best["step_apply0"]) / best["copy_table"]
    res["table_download_ms"] = 1e3 * (best["baseline"] - best["baseline_count"])
    res["table_rows_per_second"] = m / max(best["baseline_count"] - best["step_apply0"], 1e-12)
    res["host_composed_ms"] = 1e3 * sec
    res["host_composed_over_residuals_one"] = sec / best["residuals_one"]
    res["host_composed_over_baseline"] = sec / best["baseline"]
    res["max_abs_martingale_device_minus_host"] = float(np.max(np.abs(M - M_host)))
    res["max_rel_cumhaz_device_minus_host"] = float(np.max(np.abs(cols[3][:m] - cum_host) / cum_host)) if m == len(cum_host) else None
    print(json.dumps(res), flush=True)


measure(step == "post_sorted")
