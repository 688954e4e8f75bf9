"""The launch plan of cdh_glm_irls (csrc/glm_plan.hpp) restated in Python from the kernel's description of its loop (k_glm_step,
csrc/glm_kernels.hpp): a lane takes two rows per trip, a workgroup of 256 lanes a tile of 512, workgroup b the tiles b,
b + grid, ...; the rows planned are the handle's padded ld.  tests/test_glm_host.py holds it to the compiled header, and the
GPU cases (tests/test_gpu_glm.py) read from here which branch a shape reaches."""
BLOCK, VEC, MAX_GRID, VALS = 256, 2, 1024, 3
ROWS = BLOCK * VEC


def padded(n):
    """The handle's ld: n rounded up to 32 rows."""
    return -(-n // 32) * 32


def plan(n, cap=MAX_GRID):
    """-> dict(ld, vecs, tiles, grid, records, strides) for a handle of n rows."""
    ld = padded(n)
    cap = MAX_GRID if not 1 <= cap <= MAX_GRID else cap
    tiles = -(-ld // ROWS)
    grid = max(1, min(tiles, cap))
    return dict(ld=ld, vecs=ld // VEC, tiles=tiles, grid=grid, records=grid, strides=-(-tiles // grid))
