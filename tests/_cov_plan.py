"""The launch plan of the device pass loop as cov_solve() computed it before csrc/cov_plan.hpp existed, transcribed statement by
statement and in that order (each `return` is one of its `return not_now()`), with the LDS budget the launch really had; and the
two hand-counted byte formulas of its cs_alloc.  tests/test_cov_plan_host.py holds the compiled header to these."""
WIDE, FALLBACK = 134 * 1024, 36 * 1024        # dynamic LDS asked for, and what is left where the runtime refuses it
UCAP_MAX, TRACKED_MARGIN, TABLE_CAP, TABLE_MARGIN, CREW_MAX = 176, 24, 1536, 160, 64
TRACKED_BYTES = 3 * 8 + 7 * 8 + 4
TABLE_LDS = 2688 + 64 * 64 + 640
SHUFFLE_MAX_P = 5600
RUN, SUPPORT_BEYOND_TABLE, FULL_BEYOND_CAP, LIST_DOES_NOT_FIT, SHUFFLE_DOES_NOT_FIT = range(5)
INT_MAX = 0x7fffffff
CTL_BYTES = 5 * 8 + 2 * 8 + 10 * 4 + 8 + 8 + 6 * 4 + 4 * 4 + 13 * 8 + 8 + 2 * 8 + 8 * 8      # CovSolveCtl, field by field


def tri_doubles(u):
    return u * (u + 1) // 2


def lds_bytes(ucap):
    return 8 * tri_doubles(ucap) + (TRACKED_BYTES + 8) * ucap


def ucap_of(budget):
    ucap = UCAP_MAX
    while ucap > 8 and lds_bytes(ucap) > budget:
        ucap -= 4
    return ucap


def plan(p, nnz, full, randomize, budget, ucap_limit, helpers, big, support_limit):
    """-> dict: `why`, and every figure the parent had computed by the time it refused or launched"""
    out = {}
    ucap = ucap_of(budget)
    support_cap = TABLE_CAP - TABLE_MARGIN
    if nnz > support_cap:
        return dict(out, why=SUPPORT_BEYOND_TABLE)
    ucap_lists = min(ucap, ucap_limit) if ucap_limit > 0 else ucap
    lds_margin = min(TRACKED_MARGIN, ucap_lists // 4)
    nhelp = min(helpers, CREW_MAX) if (helpers > 0 and nnz + lds_margin // 2 > ucap_lists - lds_margin) else 0
    full_cap = INT_MAX if nhelp > 0 else ucap_lists - lds_margin
    out["full_cap"] = full_cap
    if full and nnz > full_cap:
        return dict(out, why=FULL_BEYOND_CAP)
    out["fold_limit"] = max(16, 120000 // p)
    out["nnz_limit"] = min(support_limit, support_cap, INT_MAX)
    tcap = TABLE_CAP
    out["ucap"] = ucap
    if tri_doubles(ucap) < TABLE_LDS:
        tcap = 0
    out["tcap"] = tcap
    if tcap == 0 and nnz > ucap - TRACKED_MARGIN:
        return dict(out, why=LIST_DOES_NOT_FIT)
    lds = lds_bytes(ucap)
    out["lds_bytes"] = lds
    if randomize and 24 * (p + 1) > lds:
        return dict(out, why=SHUFFLE_DOES_NOT_FIT)
    nh = nhelp if tcap > 0 else 0
    out["nhelp"] = nh
    out["big"] = int(tcap > 0 and (bool(big) or nh > 0 or nnz + lds_margin // 2 > ucap_lists - lds_margin))
    return dict(out, why=RUN)


def _align(v):
    return (v + 255) // 256 * 256


def dev_bytes(p):
    tc = TABLE_CAP
    return (11 * _align(8 * p) + 5 * _align(8 * p) + 12 * _align(4 * p) + 3 * _align(p) + _align(8 * p) +
            _align(8 * tc * tc) + 2 * _align(8 * tc) + _align(4 * tc) + 3 * _align(4 * p) +
            _align(CREW_BYTES) + _align(8 * p))


def pin_bytes(p):
    return _align(CTL_BYTES) + 4 * _align(4 * p) + 2 * _align(8 * p)


JOB_BYTES = 8 * 4 + 2 * 4 + 8 + 2 * 64 * 8 + 64 * 8 + 64 * 4          # CsCrewJob
CREW_BYTES = 4 * 4 + 4 * CREW_MAX + 16 * JOB_BYTES                    # CsCrew: counters, done[], the ring of 16 jobs
