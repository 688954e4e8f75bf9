"""The launch plan of the streamed sweep and of the row-summing launches beside it, restated in Python (csrc/sweep_plan.hpp): the
grids cdh_create fixes, the k_gramstep variant, chunk length and grid of a wide-block launch, the row chunks of the column
dots, the route of a chunk and its graph key, and what a chunk counts towards cdh_profile_end.

Assembled from the restatements the GPU tests carried before the header existed (test_gpu_residual_writers, test_gpu_kernel_sums,
test_gpu_feasible), which were written from the host code as it then stood in cdhip.hip (cdh_create, launch_gram_chunk, run_chunk,
col_dots, gram_launch); tests/test_sweep_plan_host.py holds the compiled header to this file.  The GPU tests size their shapes
and assert the branches they reach from here."""
import numpy as np

K_BLOCK, K_UNROLL, K_NSUM, K_COL_GROUP, K_GRAM_WAVES = 256, 4, 4, 8, 4         # kernels.hpp, gram_kernels.hpp
K_STEP_GRID_PER_CU, K_MAX_STEP_GRID, K_BLOCK_GRID_PER_CU = 8, 2048, 3
K_COL_CHUNKS, K_COL_BATCH, K_MAX_BLOCK_B, K_SHORT_ROUNDS = 64, 4096, 8, 16
K_GRAM_GRID_PER_CU, K_GRAM32_GRID_PER_CU, K_LT_GRID_PER_CU = 2, 3, 2
K_INIT_GRID_CAP, K_WEIGHTS_GRID_CAP, K_MOMENTS_GRID_CAP = 2048, 2048, 1024
K_LT_LONG_ROWS, K_WIDE64_ROWS = 2_000_000, 262_144
FRAG, LT_LONG, LT_SHORT = "frag", "lt_long", "lt_short"
VARIANT_CODE = {FRAG: 0, LT_LONG: 1, LT_SHORT: 2}

# A deliberate error for test_sweep_plan_host to plant, one at a time (None: the plan as it is):
#   "lt_per_cu_3"        three blocks per CU on the LDS-transposed path
#   "short_cut_le"       rounds64 <= kShortRounds takes short chunks
#   "grid_of_64_chunks"  the grid sized for 64-vector chunks, whatever the chunk length
FAULT = None


def _ceil(a, b):
    return -(-a // b)


def esz(dtype):
    return np.dtype(dtype).itemsize


def nv(dtype):
    return 16 // esz(dtype)                           # elements per 16-byte vector


def nvec(n, dtype):
    return _ceil(n, nv(dtype))


def gram_rec(NG):
    return NG * (NG + 1) // 2 * 256 + 16 * NG + 1     # GramRec<NG>::N: upper-triangular 16 x 16 tiles, c, q


def block_rec(B):
    return B * (B + 1) // 2 + B + 1                   # BlockRec<B>::N


# ---- what cdh_create fixes ---------------------------------------------------------------------------------------------------
def step_grid(n, dtype, cus):
    """k_step / k_axpy / k_multi_axpy (cdh_create): tiles of kBlock * kUnroll = 1024 vectors, at most min(2048, 8 / CU)."""
    return max(1, min(K_MAX_STEP_GRID, K_STEP_GRID_PER_CU * cus, _ceil(nvec(n, dtype), K_BLOCK * K_UNROLL)))


def block_grid(n, dtype, cus):
    """k_blockstep / k_block_axpy (cdh_create): strides of kBlock = 256 vectors, at most 3 blocks per CU."""
    return max(1, min(K_BLOCK_GRID_PER_CU * cus, _ceil(nvec(n, dtype), K_BLOCK)))


def elementwise_grid(n, dtype, cap):
    return max(1, min(cap, _ceil(nvec(n, dtype), K_BLOCK)))


def init_grid(n, dtype):
    """k_init_resid (rebuild_residual_from): kBlock = 256 vectors per block, capped at 2048 blocks."""
    return elementwise_grid(n, dtype, K_INIT_GRID_CAP)


def gram_blocks_per_cu(NG, use_lt):
    if use_lt:
        return 3 if FAULT == "lt_per_cu_3" else K_LT_GRID_PER_CU
    return K_GRAM32_GRID_PER_CU if NG == 2 else K_GRAM_GRID_PER_CU


def sweep_sizes(n, p, dtype, cus):
    """cdh_create: the padded column, its vectors, the visits a chunk holds, the default width, the fixed grids, the partials."""
    gram = lambda NG: cus * max(gram_blocks_per_cu(NG, False), gram_blocks_per_cu(NG, True)) * gram_rec(NG)
    return {"ld": _ceil(n, 32) * 32, "nvec": nvec(n, dtype), "cap": max(p, 4096),
            "blockB": 64 if (esz(dtype) == 8 and n < K_WIDE64_ROWS) else 32, "cus": cus,
            "step_grid": step_grid(n, dtype, cus), "block_grid": block_grid(n, dtype, cus),
            "gram_units": _ceil(nvec(n, dtype), 64 * K_GRAM_WAVES),
            "partials_doubles": max(K_MAX_STEP_GRID * K_NSUM, cus * K_BLOCK_GRID_PER_CU * block_rec(K_MAX_BLOCK_B),
                                    K_COL_BATCH * K_COL_CHUNKS * 2, gram(4), gram(2), gram(1))}


# ---- the wide-block launch ------------------------------------------------------------------------------------------------------
def gram_launch(n, dtype, B, cus, lt=2, ks=0):
    """launch_gram_chunk for block width B: the k_gramstep instantiation, its chunk length CVN (vectors), phase A's column
    groups CGN and loads per group PG, the grid G and how often the chunk loop of a wave goes round."""
    NG, f32, nvc = B // 16, esz(dtype) == 4, nvec(n, dtype)
    use_lt = (lt == 1 or (lt == 2 and (NG >= 2 or n >= K_LT_LONG_ROWS))) and not (NG == 4 and f32)
    per_cu = gram_blocks_per_cu(NG, use_lt)
    G0 = max(1, min(cus * per_cu, _ceil(nvc, 64 * K_GRAM_WAVES)))       # the grid 64-vector chunks would get
    rounds64 = _ceil(nvc, 64) // (G0 * K_GRAM_WAVES)
    cut = rounds64 <= K_SHORT_ROUNDS if FAULT == "short_cut_le" else rounds64 < K_SHORT_ROUNDS
    short = use_lt and NG > 1 and (ks == 1 or (ks == 0 and cut))        # (NG == 1 has one instantiation: KS = NG = 1)
    cvn = (64 // NG) * (1 if short else NG) if use_lt else 64
    nchunks = _ceil(nvc, cvn)
    G = G0 if FAULT == "grid_of_64_chunks" else max(1, min(cus * per_cu, _ceil(nchunks, K_GRAM_WAVES)))
    return {"variant": FRAG if not use_lt else (LT_SHORT if short else LT_LONG), "NG": NG, "CVN": cvn,
            "CGN": 64 // cvn, "PG": 8 if (use_lt and NG == 4) else (16 if NG == 4 else 8), "G": G, "Gmax": cus * per_cu,
            "nchunks": nchunks, "rounds": _ceil(nchunks, K_GRAM_WAVES * G), "ldscol": use_lt and NG == 4 and not short and not f32}


def gram_grid(n, dtype, cus):
    """cdh_gram's k_gramstep<T, 4> launch (gram_launch in cdhip.hip): blocks, and 64-vector chunks to hand out."""
    nvc = nvec(n, dtype)
    return max(1, min(cus * K_GRAM_GRID_PER_CU, _ceil(nvc, 64 * K_GRAM_WAVES))), _ceil(nvc, 64)


# ---- column dots -----------------------------------------------------------------------------------------------------------------
def col_dots_plan(bc, n, dtype, cus, width):
    """One launch over bc <= kColBatch columns: (groups of kColGroup columns, row chunks, doubles of partials at `width` per column)."""
    groups = _ceil(bc, K_COL_GROUP)
    want = max(1, _ceil(cus * 8, groups))
    chunks = max(1, min(K_COL_CHUNKS, want, _ceil(nvec(n, dtype), K_BLOCK)))
    return groups, chunks, groups * chunks * width * K_COL_GROUP


def col_dots_chunks(n, ncols, dtype, cus):
    """The row chunks of each k_col_dots / k_col_loadings launch (col_dots, col_loadings): batches of at most 4096 columns."""
    return [col_dots_plan(min(K_COL_BATCH, ncols - b0), n, dtype, cus, 2)[1] for b0 in range(0, ncols, K_COL_BATCH)]


# ---- a chunk of m visits ------------------------------------------------------------------------------------------------------------
def chunk_route(block_mode, B, has_w, m, xbits=0, dup=False):
    """run_chunk: (blocked, worth a graph, the graph's key, rewrites of r told to the residual's state)."""
    blocked = bool(block_mode) and (not has_w or B >= 16)
    key = (m << 20) | ((B if blocked else 0) << 8) | xbits | (4 if dup else 0) | (2 if has_w else 0)
    return blocked, m >= (2 * B if blocked else 8), key, (_ceil(m, B) + 1 if blocked else m + 1)


def chunk_traffic(blocked, B, m, has_w, moved, n, esz_):
    """(launches, algorithmic bytes) a streamed chunk adds to the profile; moved[i]: visit i changed its coordinate."""
    vec = float(n) * float(esz_)
    launches, nbytes = 0, 0.0
    if not blocked:
        launches += m
        for i in range(m):
            ap = i > 0 and moved[i - 1]
            nbytes += vec * ((3.0 if has_w else 2.0) + (2.0 if ap else 0.0))
        if moved[m - 1]:
            nbytes += 3.0 * vec
    else:
        for pos0 in range(0, m, B):
            nb = min(B, m - pos0)
            nzp = sum(1 for i in range(max(0, pos0 - B), pos0) if moved[i])
            nbytes += vec * (nb + 1 + nzp + (1 if nzp else 0))
            launches += 1
        nzl = sum(1 for i in range(((m - 1) // B) * B, m) if moved[i])
        if nzl:
            nbytes += vec * (nzl + 2)
    return launches, nbytes
