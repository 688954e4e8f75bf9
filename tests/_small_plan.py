"""The launch plan of the one-launch solve (csrc/small_plan.hpp) restated in Python, from the kernel's own description of its
dynamic LDS (k_solve_small, csrc/small_solve.hpp) rather than from the header's formulas; tests/test_small_plan_host.py holds
it to the compiled header, and the on-chip edge cases (tests/_onchip_edge_cases.py) read `ncache` from here."""
WIDE, DEFAULT = 160 * 1024, 64 * 1024      # the LDS of a CU where the runtime grants it, and what a kernel gets without asking
MAX_P, MAX_CACHE, MAX_LAM = 1024, 256, 64
CTL_BYTES = 8 * MAX_LAM + 4 * 4 + 8 + 2 * 8 + 8 + 2 * 4 + 3 * 8 + 2 * 4 + 8 + 2 * 4 + 8 + 2 * 8      # SmallCtl, field by field


def state_bytes(p):
    """g, beta, a, omega (doubles); list, slot2ind, ind2slot, order, draw, colslot, fyoff (p + 1), fybucket, fypar (int32);
    one int32 of padding."""
    return 4 * 8 * p + 4 * (6 * p + (p + 1) + 2 * p) + 4


def plan(p, budget=WIDE):
    """-> (fits, ncache, lds_bytes)"""
    state = state_bytes(p)
    if not 1 <= p <= MAX_P or state > budget:
        return False, 0, 0
    nc = 0
    while nc < MAX_CACHE and state + (nc + 1) * 8 * p <= budget:
        nc += 1
    return True, nc, state + nc * 8 * p


def ncache(p, budget=WIDE):
    return plan(p, budget)[1]


def unroll(p):
    """NP of k_solve_small<SQRT, NP>: the smallest of the three compiled widths whose 64 NP lanes cover p."""
    return next(w for w in (4, 8, 16) if 64 * w >= p)


def _up16(b):
    return -(-b // 16) * 16


def io_offsets(p):
    """-> (sup_off, beta_off, io_bytes) of [SmallCtl][support: p int32][beta: p doubles]"""
    sup = _up16(CTL_BYTES)
    beta = sup + _up16(4 * p)
    return sup, beta, beta + 8 * p
