"""csrc/cox_plan.hpp restated in Python: the tile, the grid, the contiguous run of tiles a workgroup owns and the scratch layout
of the Cox step.  tests/test_cox_plan_host.py holds this to the header (tests/cox_plan_main.cpp); the GPU tests read their
shapes off it."""
BLOCK, PER = 256, 4
TILE = BLOCK * PER
MAX_GRID = 1024
VALS = 5


def padded(n):
    return (n + 31) // 32 * 32


def grid_cap(cap):
    return MAX_GRID if cap < 1 or cap > MAX_GRID else cap


def plan(ld, cap=MAX_GRID):
    tiles = (ld + TILE - 1) // TILE
    grid = max(1, min(tiles, grid_cap(cap)))
    return dict(tiles=tiles, grid=grid, records=grid, longest=(tiles + grid - 1) // grid)


def run_first(tiles, grid, b):
    return b * tiles // grid


def layout(ld):
    return dict(eT=0, hA=ld, hB=2 * ld, time=3 * ld, sums=4 * ld, doubles=4 * ld + 3 * MAX_GRID, order=0, first=ld, last=2 * ld,
                ints=3 * ld)
