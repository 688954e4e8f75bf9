"""The host-only arithmetic of the solve driver, restated in Python from the loops as they stood in cdhip.hip and quad_solve.hpp
before csrc/solve_plan.hpp existed: the cold start's lambda grid and lambda_max (cdh_coordinate_descent's two branches,
quad_coordinate_descent, lambda_max), the loop of screened_full_pass, the gates of run_pass and cs_gate, gc_support_outgrown with
cov_solve's support limit, and the four lines with which solve ends a pass.  tests/test_solve_plan_host.py holds the compiled
header to this file."""
import math

K_SCREEN, K_SCREEN_MAX, K_SCREEN_MIN_PASS = 64, 1024, 16

# A deliberate error for test_solve_plan_host to plant, one at a time (None: the code as it was):
#   "grid_last_from_sum"   the grid's last entry taken from the accumulated sum l1 + numSteps * step
#   "cool_len_kept"        cool_len not reset after a screen that settled all of its columns
#   "gate_strict"          nnz * 4 < p in place of <=
FAULT = None


def _log(x):
    """std::log on doubles: -inf at 0, NaN below it and for NaN."""
    if x != x or x < 0.0:
        return math.nan
    return -math.inf if x == 0.0 else math.log(x)


def _exp(x):
    """std::exp on doubles: inf on overflow."""
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _div(a, b):
    """IEEE division of doubles (Python raises at b == 0)."""
    if b == 0.0 and a == a:
        if a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


# ---- the cold start ---------------------------------------------------------------------------------------------------------------
def cold_start_grid(lmax, target, num_steps):
    """None where the parent refuses ("... has a zero step"), else the numSteps + 1 lambdas."""
    l1, l2 = _log(lmax), _log(target)
    step = _div(l2 - l1, float(num_steps))
    if step == 0.0 or step != step:
        return None
    last = (l1 + float(num_steps) * step) if FAULT == "grid_last_from_sum" else l2
    return [_exp(last if j == num_steps else l1 + float(j) * step) for j in range(num_steps + 1)]


def lambda_max_pairs(cd, p, denom, omega):
    """lambda_max (and the one-launch branch of cdh_coordinate_descent): the dots are the even entries of the pairs."""
    lmax = 0.0
    for k in range(p):
        t = abs(_div(-cd[2 * k], denom))
        if omega is not None:
            t = _div(t, omega[k])
        if t > lmax:
            lmax = t
    return lmax


def lambda_max_quad(b, p, omega):
    """quad_coordinate_descent: max_k |b_k| / omega_k."""
    lmax = 0.0
    for k in range(p):
        t = abs(b[k])
        if omega is not None:
            t = _div(t, omega[k])
        if t > lmax:
            lmax = t
    return lmax


# ---- screened_full_pass -----------------------------------------------------------------------------------------------------------
def screen_walk(m, B, cap, p, mover):
    """The steps of screened_full_pass over m visits, in order: ("stream", pos, len) for a run_chunk, ("screen", pos, S, hit) for
    a screen of S visits whose first `hit` are settled.  mover[i]: visit i is one the screen cannot settle."""
    steps = []
    scr_max = min(K_SCREEN_MAX, p, cap)
    pos, cool, cool_len, scr = 0, 0, K_SCREEN, min(K_SCREEN, scr_max)
    while pos < m:
        if cool > 0:
            mm = min(cap, m - pos, max(cool, B))
            steps.append(("stream", pos, mm))
            pos += mm
            cool -= mm
            continue
        S = min(scr, m - pos)
        hit = S
        for i in range(S):
            if mover[pos + i]:
                hit = i
                break
        steps.append(("screen", pos, S, hit))
        pos += hit
        if hit < S:
            mm = min(max(B, 1), m - pos)
            steps.append(("stream", pos, mm))
            pos += mm
            cool = cool_len
            cool_len = min(cool_len * 2, m)
            scr = min(K_SCREEN, scr_max)
        else:
            if FAULT != "cool_len_kept":
                cool_len = K_SCREEN
            scr = min(scr * 2, scr_max)
    return steps


# ---- the gates --------------------------------------------------------------------------------------------------------------------
def run_pass_screens(screening, wls, has_w, m, nnz, p):
    """run_pass: screening && (loss != WLS || has_w) && m >= kScreenMinPass && nnz * 4 <= p."""
    dense = nnz * 4 >= p if FAULT == "gate_strict" else nnz * 4 > p
    return bool(screening) and (not wls or has_w) and m >= K_SCREEN_MIN_PASS and not dense


def cs_gate_full_goes_on(screening, wls, has_w, nnz, p):
    """cs_gate, a full pass: behind `!gc_applicable(h) || h->p < kScreenMinPass` (return), `!h->screening || nnz * 4 > p` (return)."""
    if not (not wls or has_w) or p < K_SCREEN_MIN_PASS:
        return False
    return not (not screening or nnz * 4 > p)


def weighted_and_ready(wls, has_w):
    """gc_applicable's and small_candidate's clause: loss != WLS || has_w."""
    return not wls or has_w


# ---- the rows-per-non-zero rule ---------------------------------------------------------------------------------------------------
def support_outgrown(nnz, rows_per_nnz, n_total, exempt):
    """gc_support_outgrown: the product form."""
    return False if exempt else nnz * rows_per_nnz > n_total


def support_limit(max_support, rows_per_nnz, n_total, exempt):
    """cov_solve's in.support_limit."""
    return max_support if exempt else min(max_support, n_total // rows_per_nnz)


# ---- solve's four lines -----------------------------------------------------------------------------------------------------------
def progress(maxHs, opt_tol):
    """(prev_converged, converged, iter, finished) after each pass of maxH, from the loop's start; stops where solve breaks."""
    prev, conv, it, out = False, True, 0, []
    for maxH in maxHs:
        prev = conv
        conv = maxH < opt_tol
        it += 1
        done = prev and conv
        out.append((prev, conv, it, done))
        if done:
            break
    return out
