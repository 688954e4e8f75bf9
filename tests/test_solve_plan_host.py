"""The solve driver's host-only arithmetic without a GPU (csrc/solve_plan.hpp: the cold start's lambda grid and lambda_max, the
walk of a screened full pass, the gates, the gradient cache's rows-per-non-zero rule, where the pass loop stands): compiled with
g++ -- through a ctypes shim against the Python restatement of the code these rules were taken out of (tests/_solve_plan.py), and
as a stand-alone program under the host sanitizers -- and checked by value where a number follows from arithmetic that can be
written next to it."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _solve_plan as TP

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "coordinatedescent.jl_amd", "csrc")
INF, NAN = math.inf, math.nan
STEPS = (1, 2, 50)
LMAX = (0.0, 1e-300, 0.37, 1.0, 12.5, 1e300, INF, NAN)
TARGETS = (0.0, 1e-3, 0.37 * 0.03, 0.37, np.nextafter(0.37, 1.0), 1.0, 12.5, 40.0, INF, NAN)     # above, below and equal to lmax
WALK_P = (16, 17, 63, 64, 65, 191, 192, 193, 1024, 1025, 2500, 5000)
WALK_B = (1, 8, 16, 32, 64)
DENSITIES = (0.0, 0.01, 0.1, 0.5, 1.0)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("solveplan") / "libsolveplanshim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "solve_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    i64, i32, f64, P = C.c_int64, C.c_int, C.c_double, C.POINTER
    for name, args, res in (("so_c_const", [C.c_char_p], i64), ("so_c_grid", [f64, f64, i64, P(f64)], i32),
                            ("so_c_lambda_max", [P(f64), i64, i64, f64, P(f64)], f64),
                            ("so_c_walk", [i64, i32, i64, i64, P(C.c_uint8), P(i64), i64], i64),
                            ("so_c_weights_ready", [i32, i32], i32), ("so_c_screen_gate", [i32, i32, i32, i64, i64, i64], i32),
                            ("so_c_rows_limit", [i64, i64, i32], i64), ("so_c_progress", [P(f64), i32, f64, P(i64)], i32)):
        getattr(L, name).argtypes, getattr(L, name).restype = args, res
    return L


def same(a, b):
    """== on doubles, with NaN equal to NaN."""
    return a == b or (a != a and b != b)


def c_grid(shim, lmax, target, num_steps):
    out = (C.c_double * (num_steps + 1))()
    return list(out) if shim.so_c_grid(lmax, target, num_steps, out) else None


def c_lambda_max(shim, v, stride, p, denom, omega):
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    return shim.so_c_lambda_max(pd(v), stride, p, denom, None if omega is None else pd(omega))


def c_walk(shim, m, B, cap, p, mover):
    out = np.zeros((2 * m + 2, 4), dtype=np.int64)           # a step settles or streams a visit, or is a screen that hits at once
    n = shim.so_c_walk(m, B, cap, p, mover.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_int64)), len(out))
    assert n <= len(out)
    return [("screen", int(pos), int(ln), int(hit)) if kind else ("stream", int(pos), int(ln)) for kind, pos, ln, hit in out[:n]]


def walk_cases():
    rng = np.random.default_rng(5)
    for p, B in itertools.product(WALK_P, WALK_B):
        for m in (p, p + 1, 2 * p + 3, 3 * p):
            for density in DENSITIES:
                yield p, B, m, (rng.random(m) < density).astype(np.uint8)


def test_constants(shim):
    for name, want in (("kScreen", 64), ("kScreenMax", 1024), ("kScreenMinPass", 16), ("kNoSupportLimit", 2 ** 63 - 1)):
        assert shim.so_c_const(name.encode()) == want, name
    assert (TP.K_SCREEN, TP.K_SCREEN_MAX, TP.K_SCREEN_MIN_PASS) == (64, 1024, 16)


def test_grid_is_the_parents_bit_for_bit(shim):
    refused = made = 0
    for n, lmax, target in itertools.product(STEPS, LMAX, TARGETS):
        want, got = TP.cold_start_grid(lmax, target, n), c_grid(shim, lmax, target, n)
        assert (want is None) == (got is None), (n, lmax, target)           # refused exactly where the parent refuses
        if want is None:
            refused += 1
            continue
        made += 1
        assert len(got) == n + 1 and all(same(a, b) for a, b in zip(got, want)), (n, lmax, target, got, want)
        assert same(got[-1], TP._exp(TP._log(target)))                       # the target's own logarithm, not the accumulated sum
    assert refused > 0 and made > 0
    # equal ends, a NaN at either end, and both ends at 0 or at inf (inf - inf) are refused; one end at 0 or inf is not
    for n in STEPS:
        assert c_grid(shim, 0.37, 0.37, n) is None and c_grid(shim, NAN, 0.1, n) is None and c_grid(shim, 0.37, NAN, n) is None
        assert c_grid(shim, 0.0, 0.0, n) is None and c_grid(shim, INF, INF, n) is None
        assert c_grid(shim, 0.0, 0.1, n) is not None and c_grid(shim, INF, 0.1, n) is not None
        assert c_grid(shim, 0.37, np.nextafter(0.37, 1.0), n) is not None   # one ulp apart: log tells them apart here
    # by value: 50 steps from 2 down to 0.02 is a ratio of 100^(1/50) per step
    g = c_grid(shim, 2.0, 0.02, 50)
    assert g[0] == 2.0 and g[-1] == math.exp(math.log(0.02)) and np.allclose(np.array(g[1:]) / np.array(g[:-1]), 100.0 ** (-1 / 50), rtol=1e-13, atol=0)
    # the accumulated sum would have ended elsewhere for some of these targets: the comparison above can tell
    assert any(math.exp(math.log(l) + float(n) * ((math.log(t) - math.log(l)) / float(n))) != math.exp(math.log(t))
               for n in STEPS for l in (0.37, 12.5) for t in (1e-3, 0.37 * 0.03, 40.0))


@pytest.mark.parametrize("stride", [1, 2])
def test_lambda_max_is_the_parents_loops(shim, stride):
    rng = np.random.default_rng(17 + stride)
    for p, use_omega, special in itertools.product((1, 2, 7, 64, 257), (False, True), ("none", "nan", "zero_omega", "nan_and_zero_omega")):
        dots = rng.standard_normal(p) * 10.0 ** rng.integers(-3, 4, p)
        omega = (rng.random(p) + 0.5) if use_omega else None
        if "nan" in special:
            dots[rng.integers(p)] = NAN
        if "zero_omega" in special and use_omega:
            omega[rng.integers(p)] = 0.0
        for denom in (1.0, 2500.0, math.sqrt(7.3)):
            if stride == 2:
                pairs = np.stack([dots, rng.random(p)], axis=1).ravel()          # (X_k'r, a_k)
                want, got = TP.lambda_max_pairs(pairs, p, denom, omega), c_lambda_max(shim, pairs, 2, p, denom, omega)
            else:
                if denom != 1.0:
                    continue                                                    # the quad site passes 1.0: exact
                want, got = TP.lambda_max_quad(dots, p, omega), c_lambda_max(shim, np.ascontiguousarray(dots), 1, p, 1.0, omega)
            assert got == want and got == got, (p, use_omega, special, denom, got, want)     # a NaN never wins
    one = np.array([NAN, 0.0])
    assert c_lambda_max(shim, one, 2, 1, 1.0, None) == 0.0
    assert c_lambda_max(shim, np.array([3.0, 1.0, -8.0, 1.0]), 2, 2, 2.0, np.array([1.0, 0.0])) == INF


def test_walk_is_the_parents_loop_step_by_step(shim):
    cases = 0
    for p, B, m, mover in walk_cases():
        cap = max(p, 4096)
        got, want = c_walk(shim, m, B, cap, p, mover), TP.screen_walk(m, B, cap, p, mover)
        assert got == want, (p, B, m, int(mover.sum()))
        cases += 1
        # the steps tile [0, m) in order: a screen covers the visits it settled, a stream its own
        pos = 0
        for step in got:
            assert step[1] == pos and step[2] >= 1, (p, B, m, step)
            if step[0] == "screen":
                assert step[2] <= min(1024, p) and pos + step[2] <= m and 0 <= step[3] <= step[2]
                assert not mover[pos:pos + step[3]].any() and (step[3] == step[2] or mover[pos + step[3]])
                pos += step[3]
            else:
                assert step[2] <= cap
                pos += step[2]
        assert pos == m
    assert cases == len(WALK_P) * len(WALK_B) * 4 * len(DENSITIES)


def test_walk_by_value(shim):
    quiet = lambda m: np.zeros(m, dtype=np.uint8)
    # a quiet pass at p = 5000: 64 doubling to 1024, then the rest
    assert [s[2] for s in c_walk(shim, 5000, 16, 5000, 5000, quiet(5000))] == [64, 128, 256, 512, 1024, 1024, 1024, 968]
    assert [s[2] for s in c_walk(shim, 17, 16, 4096, 17, quiet(17))] == [17]                 # never more than p columns ...
    assert [s[2] for s in c_walk(shim, 51, 16, 4096, 17, quiet(51))] == [17, 17, 17]         # ... however long the pass
    # one mover at visit 70 of 700, B = 16: the screen of 128 behind the first 64 settles 6, the mover streams with its block of
    # 16, the next 64 visits stream unscreened (max(cool, B)), and the screens start again at 64
    mover = quiet(700)
    mover[70] = 1
    assert c_walk(shim, 700, 16, 4096, 700, mover)[:6] == [("screen", 0, 64, 64), ("screen", 64, 128, 6), ("stream", 70, 16), ("stream", 86, 64),
                                                          ("screen", 150, 64, 64), ("screen", 214, 128, 128)]
    # everything moves, B = 1, m = p = 193: each miss doubles the cool-down, 64 -> 128, capped by what is left of the pass
    assert c_walk(shim, 193, 1, 4096, 193, np.ones(193, dtype=np.uint8)) == [
        ("screen", 0, 64, 0), ("stream", 0, 1), ("stream", 1, 64), ("screen", 65, 64, 0), ("stream", 65, 1), ("stream", 66, 127)]
    # the visit after a hit streams max(B, 1) visits: at B = 64 a pass of 3 p = 48 visits over p = 16 columns is over with it
    steps = c_walk(shim, 48, 64, 4096, 16, np.ones(48, dtype=np.uint8))
    assert steps == [("screen", 0, 16, 0), ("stream", 0, 48)]


def test_gates_limit_and_progress_are_the_parents(shim):
    for screening, wls, has_w, nnz in itertools.product((0, 1, 2), (0, 1), (0, 1), range(0, 12)):
        assert bool(shim.so_c_weights_ready(wls, has_w)) == TP.weighted_and_ready(wls, has_w)
        for p in (15, 16, 17, 20, 40):
            for m in (p, 15, 16, 3 * p):
                assert bool(shim.so_c_screen_gate(screening, wls, has_w, m, nnz, p)) == TP.run_pass_screens(screening, wls, has_w, m, nnz, p), (screening, wls, has_w, m, nnz, p)
            # cs_gate asks about the p visits of a full pass, behind gc_applicable and p >= kScreenMinPass
            if TP.weighted_and_ready(wls, has_w) and p >= TP.K_SCREEN_MIN_PASS:
                assert bool(shim.so_c_screen_gate(screening, wls, has_w, p, nnz, p)) == TP.cs_gate_full_goes_on(screening, wls, has_w, nnz, p)
    assert shim.so_c_screen_gate(1, 0, 0, 16, 4, 16) and not shim.so_c_screen_gate(1, 0, 0, 16, 5, 16) and not shim.so_c_screen_gate(1, 0, 0, 15, 0, 15)
    for r, n, exempt in itertools.product((1, 2, 32, 400), (1, 31, 32, 33, 399, 400, 401, 3000, 10_000_019), (0, 1)):
        limit = shim.so_c_rows_limit(n, r, exempt)
        for max_support in (512, 4096):
            assert min(max_support, limit) == TP.support_limit(max_support, r, n, exempt)
        for nnz in range(max(0, n // r - 3), n // r + 4):                  # the limit form is the product form
            assert (nnz > limit) == TP.support_outgrown(nnz, r, n, exempt) == (not exempt and nnz * r > n), (r, n, exempt, nnz)
    out = (C.c_int64 * 24)()
    for length in range(1, 7):
        for below in itertools.product((False, True), repeat=length):
            maxH = [1e-13 if b else 1e-3 for b in below]
            n = shim.so_c_progress((C.c_double * length)(*maxH), length, 1e-12, out)
            got = [(bool(out[4 * k]), bool(out[4 * k + 1]), out[4 * k + 2], bool(out[4 * k + 3])) for k in range(n)]
            assert got == TP.progress(maxH, 1e-12), below
    assert TP.progress([1e-13], 1e-12) == [(True, True, 1, True)]           # the loop starts `converged`: one quiet full pass ends it


@pytest.mark.parametrize("fault", ["grid_last_from_sum", "cool_len_kept", "gate_strict"])
def test_a_planted_error_fails_the_comparison(shim, monkeypatch, fault):
    """The comparisons are fine enough to tell the header from a twin with one rule wrong."""
    def mismatches():
        grid = sum(not all(same(a, b) for a, b in zip(c_grid(shim, l, t, n), TP.cold_start_grid(l, t, n)))
                   for n in STEPS for l in (0.37, 12.5) for t in (1e-3, 0.37 * 0.03, 40.0))
        walk = sum(c_walk(shim, m, B, max(p, 4096), p, mover) != TP.screen_walk(m, B, max(p, 4096), p, mover)
                   for p, B, m, mover in walk_cases() if p in (193, 1025) and B in (1, 16))
        gate = sum(bool(shim.so_c_screen_gate(1, 0, 0, p, nnz, p)) != TP.run_pass_screens(1, 0, 0, p, nnz, p) for p in (16, 17, 20, 40) for nnz in range(12))
        return grid, walk, gate
    assert mismatches() == (0, 0, 0)
    monkeypatch.setattr(TP, "FAULT", fault)
    got = mismatches()
    assert got[("grid_last_from_sum", "cool_len_kept", "gate_strict").index(fault)] > 0 and sum(g > 0 for g in got) == 1, got


def test_sanitized_stand_alone_program(tmp_path):
    exe = str(tmp_path / "solve_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "solve_plan_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "solve_plan_main OK" in out


def test_the_driver_and_its_rules_have_one_home():
    strip = lambda t: re.sub(r"//[^\n]*", "", t)
    plan = strip(open(os.path.join(CSRC, "solve_plan.hpp")).read())
    assert not re.search(r"hip|__global__|__device__|__host__|__shared__|threadIdx|blockIdx", plan, flags=re.I)
    assert re.findall(r"#include\s*\"([^\"]+)\"", plan) == []
    src = {f: strip(open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".h"))}
    others = "".join(t for f, t in src.items() if f != "solve_plan.hpp")
    # one grid, one reduction, one gate, one support rule, one constant each
    assert "std::log(" in plan and not re.search(r"std::log\((lmax|target|l\w*ambda|q->h_lambda0)", others)
    assert others.count("cold_start_grid(") == 2 and others.count("lambda_max_of(") == 3         # (solve.hpp's head of a cold start serves two routes)
    assert "has a zero step" in src["solve.hpp"] and src["solve.hpp"].count("has a zero step") == 1 and src["cdhip.hip"].count("has a zero step") == 0
    assert "of a problem has a zero step" in src["quad_solve.hpp"]
    assert "nnz() * 4" not in others and "nnz * 4 <= p" in plan
    assert not re.search(r"\bkScreen(Max)?\b", others) and others.count("kScreenMinPass") == 1   # cs_gate's own p >= kScreenMinPass
    assert others.count("screen_gate(") == 1 and others.count("full_pass_screened(") == 3        # its definition, run_pass, cs_gate
    assert not re.search(r"loss != CDH_WLS \|\| h->has_w", others) and others.count("weights_ready(") == 2
    assert others.count("rows_support_limit(") == 1 and "gc_rows_per_nnz(h) >" not in others and "/ gc_rows_per_nnz(h)" not in others
    assert not re.search(r"bool\s*\*\s*prev_conv|int64_t\s*\*\s*iter", others)
    # the driver stands in solve.hpp, the exports call it, and the include stands where screened_full_pass stood
    hip, drv = src["cdhip.hip"], src["solve.hpp"]
    for name in ("screened_full_pass", "run_pass", "solve", "descend", "pass", "solve_once", "coordinate_descent"):
        assert re.search(r"^int32_t %s\(" % name, drv, flags=re.M) and not re.search(r"^int32_t %s\(" % name, hip, flags=re.M), name
    for call in ("return descend(h, k1, out_h);", "return pass(h, m, idx1, out_maxH);", "return solve_once(h, opt, out);", "return coordinate_descent(h, opt, out);"):
        assert hip.count(call) == 1, call
    assert hip.count('#include "solve.hpp"') == 1
    assert hip.index('#include "glm_kernels.hpp"') < hip.index('#include "solve.hpp"') < hip.index("void free_all(")
    assert "kGcRowsPerNnz" not in hip and "constexpr int64_t kGcRowsPerNnz = 400;" in src["grad_cache.hpp"]
