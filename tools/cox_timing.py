#!/usr/bin/env python3
"""The Cox step against its yardsticks, and CoxLassoPath against the same loop composed on the host.  Prints ONE JSON line.

Run without arguments it is a driver: every measurement below runs in a child process of its own under `timeout -k 10`, in
order, and nothing runs after a child that failed or timed out (its status is in the line).  With --step NAME it is that child.

  step_random, step_sorted   cdh_glm_cox_irls(apply = 1) -- and apply = 0 -- on an fp64 handle of N rows (default 2 000 000)
      and one column, with an offset, times rounded to three decimals (tie groups of a few hundred rows), three rows in ten
      censored; rows in random time order, or pre-sorted by time.  Against (i) a device-to-device copy of the bytes the chain
      of launches moves, 228 a row: exp 52 (order, y, r, offset, status in; e and the status out), suffix scan 16, hazards
      36 (status, first, S in; h, h2 out), prefix scans 32, apply 92 (order, first, last 12; y, r, offset, status 32; S, A, B
      24 in; w, y, r 24 out) -- the copy reads and writes 114 N bytes; gathers and scatters through the order move whole 64-byte
      sectors for 8 useful bytes when the rows are in random order, which the count does not include; and (ii) the same step
      composed on the host: cdh_get_residual, the twin's formulas in numpy with the sort order cached (cumulative sums in
      sorted order), cdh_set_y and cdh_set_obs_weights.  Interleaved call by call, REPS calls each per round, ROUNDS rounds;
      reported are the rounds' minima, their minimum and spread.  Times are host clocks around calls that end in a stream
      synchronise.
  path   CoxLassoPath (default N2 = 2 000 000, P2 = 1000, M2 = 30 lambdas from 0.9 to 0.05 of lambda_max, with an offset, IRLS
      optTol 1e-7) against the same warm-started loop composed from cdh_get_residual, numpy, cdh_set_y, cdh_set_obs_weights
      and cdh_initialize per round, on one handle, PROUNDS rounds after a warm-up of each on the first three lambdas;
      reported: wall times, the IRLS rounds of each, whether they agree at every lambda, the largest difference of the
      coefficients.

STRATA=S (default 0: everything above, unchanged) runs the same three measurements with S strata (ids uniform over the rows) and
observation weights uniform in [0.25, 4], normalised to sum to n, through cdh_glm_set_survival_strata: "pre-sorted" is then by
(stratum, time), the host's step takes its cumulative sums per stratum, and the copy moves 252 bytes a row -- the weight is
gathered in the exp and the apply launch (16) and one int32 stratum bound is read in each of the two scan launches (8).  The
line gains the keys "strata" and "weighted" in every measurement.

INTERVAL=1 (default 0) adds start times -- start = time x U(0, 0.9) floored to three decimals, 0 for three rows in ten; the times
are then at least 0.001 -- through cdh_glm_set_survival_interval, with STRATA's strata and weights or, with STRATA=0, one
stratum and unit weights (the interval handle runs the segmented, weighted chain either way).  The host's step keeps the second
order and the two lookups cached.  The copy moves 336 bytes a row, the strata step's 252 and 84 more: the gather of ev into the
start order 20 (pos2 4, ev in 8, T2 out 8), T2's suffix scan 20 (16 and the stratum bound 4), the hazards 12 (lo 4, T2 8), the
apply launch 32 (lo and enter 8, T2 8, the hazards' prefix sums at the entry 16).  Of these pos2 and enter are gathers in random
order whatever the rows' order; lo is monotone inside a stratum.  The line gains the key "interval".

EFRON=1 (default 0; not with INTERVAL) sets the handle to Efron ties (cdh_glm_set_cox_ties) after the survival data: the step
measured is Efron's, and the Breslow step OF THE SAME HANDLE is timed beside it call by call ("breslow_apply1": the rule is set
before each call, a host-side flag once the Efron scratch exists), so the line carries "efron_over_breslow" next to
"efron_bytes_over_breslow_bytes", the ratio the byte counts predict.  Efron's chain always runs the segmented, weighted
arithmetic; over the strata step's 252 bytes a row it moves 260 more, 512: the mark launch 48 (ev, dv, first, last in; cnt, Dv,
Sdv out), the three tie-group scans 56 (16 each and their bounds 4 + 4), the hazard launch 68 (last, cnt twice, Dv, Sdv in; hc,
hc2, lg, mm out), the scan of (hc, hc2) 36, the apply launch 52 (sfirst, the prefix sums in front of the group 16, hc and hc2 at
its end 16, lg, mm -- less S, which it no longer reads, 8 -- the count takes the event rows' reads for every row).  DECIMALS
(default 3) is the rounding of the times: 4 ties about half of the events at n = 2 000 000 with 100 strata; the line reports the
fraction that is tied ("tied_events").  The host's step is then the Efron twin's (tests/_cox_efron_numpy.py) in its
cumulative-sum form, the tie groups' sums as differences of cumulative sums.

Environment: N, REPS, ROUNDS, N2, P2, M2, PROUNDS, STEP_TIMEOUT, PATH_TIMEOUT, STRATA, INTERVAL, EFRON, DECIMALS, OUT (a file that
receives the line too)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
env = lambda k, d: int(os.environ.get(k, d))  # noqa: E731
STEPS = ("step_random", "step_sorted", "path")


def driver():
    res, ok = {}, True
    for name in STEPS:
        if not ok:
            res[name] = {"skipped": "an earlier step failed"}
            continue
        limit = env("PATH_TIMEOUT", 600) if name == "path" else env("STEP_TIMEOUT", 180)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        last = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not last:
            res[name] = {"failed": p.returncode, "stderr_tail": p.stderr[-400:]}
            ok = False
        else:
            res[name] = json.loads(last[-1])
        print("cox_timing: %s %s" % (name, "done" if ok else "failed"), file=sys.stderr, flush=True)
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
import coordinatedescent_jl_amd as cd  # noqa: E402

step = sys.argv[sys.argv.index("--step") + 1]
vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
PD = C.POINTER(C.c_double)
WMIN, ETA_MAX = 1e-5, 50.0
STRATA = env("STRATA", 0)
INTERVAL = env("INTERVAL", 0)
EFRON = env("EFRON", 0)
DECIMALS = env("DECIMALS", 3)
BRESLOW_BYTES = 336 if INTERVAL else (252 if STRATA else 228)
BYTES = 512 if EFRON else BRESLOW_BYTES
assert not (EFRON and INTERVAL), "Efron ties are not offered with start-stop times"


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


class HostStep:
    """The twin's step (tests/_cox_numpy.py: rows, the cumulative-sum form) with the sort order and the tie groups cached.
    With strata g and weights v (tests/_cox_strata_numpy.py) the order is by (stratum, time) and a cumulative sum restarts
    at a stratum's boundary: the sum over all positions less its value just outside the stratum.  With start times
    (tests/_cox_interval_numpy.py) a second order by (stratum, start) and the two lookups lo and enter are cached too."""

    def __init__(self, t, status, off, g=None, v=None, start=None):
        n = len(t)
        if start is not None and g is None:
            g = np.zeros(n, dtype=np.int32)
        self.order = np.argsort(t, kind="stable") if g is None else np.lexsort((t, g))
        ts = t[self.order]
        head = np.r_[True, ts[1:] != ts[:-1]]
        self.sfirst = self.slast = None
        if g is not None:
            gs = g[self.order]
            shead = np.r_[True, gs[1:] != gs[:-1]]
            head |= shead
            sstarts = np.nonzero(shead)[0]
            sid = np.cumsum(shead) - 1
            self.sfirst, self.slast = sstarts[sid], (np.r_[sstarts[1:], n] - 1)[sid]
        starts = np.nonzero(head)[0]
        gid = np.cumsum(head) - 1
        self.first, self.last = starts[gid], (np.r_[starts[1:], n] - 1)[gid]
        self.v = np.ones(n) if v is None else v
        self.dv = self.v * status
        self.ds, self.off = self.dv[self.order], off
        self.inv = np.empty(n, dtype=np.int64)
        self.inv[self.order] = np.arange(n)
        self.order2 = None
        if start is not None:
            self.order2 = np.lexsort((start, g))
            self.lo, self.enter = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
            s2, u = start[self.order2], start[self.order]
            for a, b in zip(sstarts.tolist(), (np.r_[sstarts[1:], n] - 1).tolist()):
                lo = np.searchsorted(s2[a:b + 1], ts[a:b + 1], side="left")
                self.lo[a:b + 1] = np.where(lo <= b - a, a + lo, -1)
                en = np.searchsorted(ts[a:b + 1], u[a:b + 1], side="right") - 1
                self.enter[a:b + 1] = np.where(en >= 0, a + en, -1)
            self.has_lo, self.has_enter = self.lo >= 0, self.enter >= 0
            self.lo, self.enter = np.maximum(self.lo, 0), np.maximum(self.enter, 0)

    def _suffix(self, a):
        T = np.cumsum(a[::-1])[::-1]
        return T if self.slast is None else T - np.r_[T[1:], 0.0][self.slast]

    def _prefix(self, a):
        c = np.cumsum(a)
        return c if self.sfirst is None else c - np.r_[0.0, c[:-1]][self.sfirst]

    def _efron(self, e):
        """The Efron twin's A and B per row (tests/_cox_efron_numpy.py, scans): a sum over a tie group is the difference of a
        cumulative sum at its bounds."""
        first, last = self.first, self.last
        es, ds = e[self.order], self.ds
        event = ds != 0.0

        def group_prefix(a):
            c = np.cumsum(a)
            return c - np.r_[0.0, c[:-1]][first]

        cnt, Dv, Sdv = group_prefix(event.astype(np.float64)), group_prefix(np.where(event, es, 0.0)), group_prefix(ds)
        d, D, S = cnt[last], Dv[last], self._suffix(es)[first]
        with np.errstate(divide="ignore", invalid="ignore"):
            m = Sdv[last] / d
            frac = (cnt - 1.0) / d
            den = S - frac * D
            ok = event & (den > 0.0)
            cf = 1.0 - frac
            h = np.where(ok, m / den, 0.0)
            h2 = np.where(ok, h / den, 0.0)
            hc, hc2 = np.where(ok, cf * h, 0.0), np.where(ok, (cf * cf) * h2, 0.0)
        if self.sfirst is None:
            cA, cB, some = np.cumsum(h), np.cumsum(h2), first > 0
        else:
            cA, cB, some = self._prefix(h), self._prefix(h2), first > self.sfirst
        before = np.maximum(first - 1, 0)
        A = np.where(event, np.where(some, cA[before], 0.0) + group_prefix(hc)[last], cA[last])
        B = np.where(event, np.where(some, cB[before], 0.0) + group_prefix(hc2)[last], cB[last])
        return A[self.inv], B[self.inv]

    def __call__(self, eta_lin):
        e = self.v * np.exp(np.minimum(eta_lin + self.off, ETA_MAX))
        if EFRON:
            A, B = self._efron(e)
            eA = e * A
            w = np.maximum(eA - e * (e * B), WMIN)
            return eta_lin + (self.dv - eA) / w, w
        Ss = self._suffix(e[self.order])[self.first]
        if self.order2 is not None:
            Ss = Ss - np.where(self.has_lo, self._suffix(e[self.order2])[self.lo], 0.0)
        h = self.ds / Ss
        cA, cB = self._prefix(h), self._prefix(h / Ss)
        A, B = cA[self.last], cB[self.last]
        if self.order2 is not None:
            A, B = A - np.where(self.has_enter, cA[self.enter], 0.0), B - np.where(self.has_enter, cB[self.enter], 0.0)
        A, B = A[self.inv], B[self.inv]
        eA = e * A
        w = np.maximum(eA - e * (e * B), WMIN)
        return eta_lin + (self.dv - eA) / w, w


def survival(f, seed, presorted):
    """Times ~ Exp(1) / exp(signal), rounded to three decimals; 30 % censored; an offset in (-0.5, 0.5).  With STRATA: ids
    uniform over the rows and weights uniform in [0.25, 4], normalised to sum to n.  With INTERVAL: start times (the module's
    docstring).  -> (t, status, off, strata, weights, start)."""
    n = f.n
    rng = np.random.default_rng(seed)
    sig = f.y
    off = rng.uniform(-0.5, 0.5, n)
    t = np.round(rng.exponential(1.0, n) / np.exp(0.5 * sig / np.std(sig) + off), DECIMALS)
    status = (rng.random(n) >= 0.3).astype(np.float64)
    if INTERVAL:
        t = np.maximum(t, 0.001)

    def starts(t):
        if not INTERVAL:
            return None
        r2 = np.random.default_rng(seed + 1000)
        return np.where(r2.random(n) < 0.3, 0.0, np.floor(t * r2.uniform(0.0, 0.9, n) * 1000.0) / 1000.0)

    if not STRATA:
        if presorted:
            t = np.sort(t)
        start = starts(t)
        set_survival(f, t, status, off, None, None, start)
        return t, status, off, None, None, start
    g = rng.integers(0, STRATA, n).astype(np.int32)
    v = rng.uniform(0.25, 4.0, n)
    v = v * n / v.sum()
    if presorted:
        o = np.lexsort((t, g))
        t, g = np.ascontiguousarray(t[o]), np.ascontiguousarray(g[o])
    start = starts(t)
    set_survival(f, t, status, off, g, v, start)
    f._weighted = True
    return t, status, off, g, v, start


def set_survival(f, t, status, off, g, v, start=None):
    _set_survival(f, t, status, off, g, v, start)
    if EFRON:                                                   # (the setters keep the rule; the first call allocates its scratch)
        cd.check(f._L.cdh_glm_set_cox_ties(f._h, 1), f._h)


def tied_events(t, status, g):
    """The fraction of the events that share their time (and stratum) with another event."""
    ev = status != 0
    key = t[ev] if g is None else np.stack([g[ev].astype(np.float64), t[ev]], axis=1)
    _, inv, cnt = np.unique(key, axis=0 if g is not None else None, return_inverse=True, return_counts=True)
    return float((cnt[inv.ravel()] > 1).mean())


def _set_survival(f, t, status, off, g, v, start=None):
    if start is not None:
        cd.check(f._L.cdh_glm_set_survival_interval(f._h, vp(start), vp(t), vp(status), vp(off), None if g is None else vp(g),
                                                    None if v is None else vp(v)), f._h)
    elif g is None:
        cd.check(f._L.cdh_glm_set_survival(f._h, vp(t), vp(status), vp(off)), f._h)
    else:
        cd.check(f._L.cdh_glm_set_survival_strata(f._h, vp(t), vp(status), vp(off), vp(g), vp(v)), f._h)


def measure_step(presorted):
    n, reps, rounds = env("N", 2_000_000), env("REPS", 5), env("ROUNDS", 3)
    f, _ = cd.CDCoxLoss.generate(n, 1, seed=7, s=1, noise=1.0)
    t, status, off, g, v, start = survival(f, 7, presorted)
    x = cd.SparseIterate(1)
    x[1] = 0.5
    cd.initialize_(f, x)
    L, h = f._L, f._h
    out5, r = np.zeros(5), np.zeros(n)
    host = HostStep(t, status, off, g, v, start)
    z = f.y

    def dev1():
        cd.check(L.cdh_glm_cox_irls(h, -1, 1, WMIN, ETA_MAX, out5.ctypes.data_as(PD)), h)

    def dev0():
        cd.check(L.cdh_glm_cox_irls(h, -1, 0, WMIN, ETA_MAX, out5.ctypes.data_as(PD)), h)

    def breslow1():                                             # the Breslow step of the same handle, the rule restored after it
        cd.check(L.cdh_glm_set_cox_ties(h, 0), h)
        cd.check(L.cdh_glm_cox_irls(h, -1, 1, WMIN, ETA_MAX, out5.ctypes.data_as(PD)), h)
        cd.check(L.cdh_glm_set_cox_ties(h, 1), h)

    def composed():
        nonlocal z
        cd.check(L.cdh_get_residual(h, vp(r)), h)
        z, w = host(z - r)
        cd.check(L.cdh_set_y(h, vp(z)), h)
        cd.check(L.cdh_set_obs_weights(h, vp(w)), h)

    src = torch.randn(BYTES // 2 * n // 8, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    names, fns = ("cox_apply1", "cox_apply0", "copy_%d_bytes_a_row" % BYTES), (dev1, dev0, copy)
    if EFRON:
        names, fns = names + ("breslow_apply1",), fns + (breslow1,)
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
    # the composed step last: it replaces y and w from the host and leaves r for the next catch-up
    comp = []
    for _ in range(max(2, rounds)):
        f._synced = None
        cd.initialize_(f, x)
        z = f.y
        comp.append(timed(composed)[0])
    res = {"n": n, "presorted": presorted, "tie_groups": int(len(np.unique(t))), "clamped": int(out5[2]),
           "events": float(out5[4]) if STRATA else int(out5[4]), "bytes_a_row": BYTES, "strata": STRATA, "weighted": bool(STRATA), "interval": INTERVAL}
    for k, v in per.items():
        res[k] = {"round_minima_ms": [1e3 * a for a in v], "min_ms": 1e3 * min(v), "spread_ms": 1e3 * (max(v) - min(v)),
                  "TBps_of_%dn" % BYTES: BYTES * n / min(v) / 1e12}
    res["host_composed_ms"] = [1e3 * a for a in comp]
    res["cox_over_copy"] = min(per[names[0]]) / min(per[names[2]])
    res["efron"] = EFRON
    res["tied_events"] = tied_events(t, status, g)
    if EFRON:
        res["efron_over_breslow"] = min(per["cox_apply1"]) / min(per["breslow_apply1"])
        res["efron_bytes_over_breslow_bytes"] = BYTES / BRESLOW_BYTES
    res["host_composed_over_cox"] = min(comp) / min(per[names[0]])
    f.close()
    return res


def measure_path():
    n, p, m, rounds = env("N2", 2_000_000), env("P2", 1000), env("M2", 30), env("PROUNDS", 2)
    f, _ = cd.CDCoxLoss.generate(n, p, seed=11, s=10, noise=1.0)
    t, status, off, g, v, start = survival(f, 11, False)
    lmax = cd.coxLambdaMax(f)
    lam = lmax * np.geomspace(0.9, 0.05, m)
    opts = cd.CDOptions(maxIter=2000, optTol=1e-7, randomize=False)
    irls = cd.IRLSOptions(maxIter=100)
    host = HostStep(t, status, off, g, v, start)
    L, h = f._L, f._h

    def device_route(lams):
        return cd.CoxLassoPath(f, None, lams, opts, irls, standardizeX=False, **({"ties": "efron"} if EFRON else {}))

    def composed_route(lams):
        x, betas, rounds_, r = cd.SparseIterate(p), [], [], np.zeros(n)
        z = np.zeros(n)
        cd.check(L.cdh_set_y(h, vp(z)), h)
        f._synced = None
        cd.initialize_(f, x)
        mode = f.gradient_cache_mode()
        if mode == 1:
            f.set_gradient_cache(2)
        try:
            for lj in lams:
                g_, beta, k = cd.ProxL1(lj), x.dense(), 0
                for k in range(1, irls.maxIter + 1):
                    cd.check(L.cdh_get_residual(h, vp(r)), h)
                    z, w = host(z - r)
                    cd.check(L.cdh_set_y(h, vp(z)), h)
                    cd.check(L.cdh_set_obs_weights(h, vp(w)), h)
                    f._synced = None
                    cd.initialize_(f, x)
                    cd.coordinateDescent_(x, f, g_, opts)
                    beta, old = x.dense(), beta
                    if np.max(np.abs(beta - old)) < irls.optTol:
                        break
                betas.append(beta)
                rounds_.append(k)
        finally:
            if mode == 1:
                f.set_gradient_cache(1)
        return betas, rounds_

    def reset():
        set_survival(f, t, status, off, g, v, start)            # the Cox handle as it was made: y = r = 0
        f._synced = None

    device_route(lam[:3])
    reset()
    composed_route(lam[:3])
    t_dev, t_com = [], []
    for _ in range(rounds):
        reset()
        tt, path = timed(lambda: device_route(lam))
        t_dev.append(tt)
        reset()
        tt, (betas, crounds) = timed(lambda: composed_route(lam))
        t_com.append(tt)
    diff = max(float(np.max(np.abs(b.dense() - c))) for b, c in zip(path.betapath, betas))
    res = {"n": n, "p": p, "lambdas": m, "strata": STRATA, "weighted": bool(STRATA), "interval": INTERVAL, "efron": EFRON, "CoxLassoPath_s": t_dev, "composed_s": t_com,
           "min_s": {"CoxLassoPath": min(t_dev), "composed": min(t_com)},
           "composed_over_CoxLassoPath": min(t_com) / min(t_dev),
           "irls_rounds": {"CoxLassoPath": int(sum(path.rounds)), "composed": int(sum(crounds))},
           "same_rounds_per_lambda": list(path.rounds) == list(crounds), "all_converged": bool(all(path.converged)),
           "nnz_last": int(path.betapath[-1].nnz), "max_abs_diff_beta": diff}
    f.close()
    return res


out = measure_path() if step == "path" else measure_step(step == "step_sorted")
print(json.dumps(out), flush=True)
