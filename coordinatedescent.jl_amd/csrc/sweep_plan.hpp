// sweep_plan.hpp -- the host-only arithmetic of the streamed sweep (sweep.hpp: run_chunk and its three launchers) and of the
// row-summing launches beside it (col_dots, col_loadings, vc_point, resid_moments_dev, cdh_gram): what cdh_create sizes, which
// k_gramstep instantiation a chunk runs and on what grid, the fixed grids of k_step and k_blockstep, the row chunks of the
// column dots, whether a chunk is replayed from a graph and under which key, and what a chunk counts towards
// cdh_profile_end.  No HIP in here: tests/test_sweep_plan_host.py compiles it with g++ (tests/sweep_plan_main.cpp) and holds it
// to tests/_sweep_plan.py.  The launchers call these functions and nothing else decides the numbers.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- what the kernels fix (kernels.hpp, gram_kernels.hpp) and the two sizes of col_dots' batch loop (cdhip.hip), restated:
// cdhip.hip ties each to the name it has there ------------------------------------------------------------------------------------
constexpr int kSpBlock = 256;      // kBlock: lanes of the vector-ALU kernels, one 16-byte vector each per trip
constexpr int kSpUnroll = 4;       // kUnroll: vectors a lane of k_step has in flight
constexpr int kSpNSum = 4;         // kNSum: doubles of a k_step partial record
constexpr int kSpColGroup = 8;     // kColGroup: columns a k_col_dots block takes
constexpr int kSpGramWaves = 4;    // kGramWaves: waves of a k_gramstep block, a chunk each per round
constexpr int kSpGramChunk = 64;   // vectors of a fragment-path chunk; the LDS-transposed chunks are 64 / NG sub-chunks of it
constexpr int kSpColChunks = 64;       // kColChunks
constexpr int64_t kSpColBatch = 4096;  // kColBatch
constexpr int64_t sp_gram_rec(int NG) { return (int64_t)NG * (NG + 1) / 2 * 256 + 16 * NG + 1; }   // GramRec<NG>::N
constexpr int64_t sp_block_rec(int B) { return (int64_t)B * (B + 1) / 2 + B + 1; }                 // BlockRec<B>::N

// ---- the launch policy's own constants ------------------------------------------------------------------------------------------
constexpr int kStepGridPerCU = 8;    // blocks per CU of k_step (and the axpy kernels that share its grid)
constexpr int kMaxStepGrid = 2048;   // blocks of k_step (8 per CU on 256 CUs)
constexpr int kBlockGridPerCU = 3;   // blocks per CU of k_blockstep
constexpr int kColFillPerCU = 8;     // blocks per CU a k_col_dots launch aims for
constexpr int kMaxBlockB = 8;
constexpr int kShortRounds = 16;     // below this many rounds of 64-vector chunks per launch: short chunks
// blocks of k_gramstep per CU: as many as stay resident for the variant launched (register footprint: B = 64 holds 2 waves per
// SIMD, the narrower ones 3; the LDS-transposed variants are bounded by their 68-78 KB operand tiles to 2 blocks -- B = 32
// launched with 3 per CU ran its third of the grid as a second, half-empty round: 933 -> 861 us per block at 1e7 rows), never
// more than the partial buffer was sized for
constexpr int kGramGridPerCU = 2;     // fragment path, B = 16 and 64
constexpr int kGram32GridPerCU = 3;   // fragment path, B = 32
constexpr int kLtGridPerCU = 2;       // LDS-transposed path, every width
constexpr int64_t kLtLongRows = 2000000;   // B = 16 takes the LDS-transposed path from this many rows on
// The default sweep width: B = 32 streams fastest per visit on long columns; on SHORT ones (the grid is not even full: fewer
// than 512 blocks x 4 waves x 64 vectors) a block of visits costs three launches whatever it reads, and B = 64 halves them
// (benchmark/cd_bench.jl's dense solve at n = 3000: 0.40 s at B = 32, 0.26 s at B = 64).  fp32 storage has no LDS-transposed
// B = 64 kernel and keeps 32.
constexpr int64_t kWide64Rows = (int64_t)512 * kSpGramWaves * kSpGramChunk * 2;
// caps of the elementwise grids (elementwise_grid)
constexpr int64_t kInitGridCap = 2048;      // k_init_resid
constexpr int64_t kWeightsGridCap = 2048;   // k_vc_weights
constexpr int64_t kMomentsGridCap = 1024;   // k_resid_moments: its records are summed by one block

constexpr int64_t sp_min(int64_t a, int64_t b) { return a < b ? a : b; }
constexpr int64_t sp_max(int64_t a, int64_t b) { return a > b ? a : b; }
constexpr int64_t sp_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Grid size for a grid-stride kernel with `units` work items and at most `gmax` resident blocks.
// Measured: keeping every CU slot occupied (gmax blocks) beats equalising per-block work -- the streaming rate is set per CU
// (~24 GB/s each), so an idle slot costs more than a block that runs one iteration longer.
constexpr int balanced_grid(int64_t units, int64_t gmax) { return (int)sp_max(1, sp_min(gmax, units)); }

// min(cap, ceil(nvec / kBlock)), at least 1: k_init_resid, k_vc_weights, k_resid_moments
constexpr int elementwise_grid(int64_t nvec, int64_t cap) { return balanced_grid(sp_ceil(nvec, kSpBlock), cap); }

constexpr int gram_blocks_per_cu(int NG, bool lt) { return lt ? kLtGridPerCU : NG == 2 ? kGram32GridPerCU : kGramGridPerCU; }

// ---- what cdh_create derives ------------------------------------------------------------------------------------------------------
struct SweepSizes {
    int64_t ld;          // rows of a column as stored: every column starts 128/256-B aligned
    int64_t nvec;        // 16-byte vectors over the n rows; pad rows [n, ld) are zero in X, y, r, w
    int64_t cap;         // visits per chunk
    int blockB;          // the default sweep width
    int cus;
    int step_grid;       // k_step, k_axpy, k_multi_axpy
    int block_grid;      // k_blockstep, k_block_axpy
    int64_t gram_units;  // units of kGramWaves fragment-path chunks
    size_t partials_doubles;
};
constexpr SweepSizes sweep_sizes(bool f64, int64_t n_local, int64_t p, int cus) {
    const int NV = f64 ? 2 : 4;
    SweepSizes s{};
    s.ld = sp_ceil(n_local, 32) * 32;
    s.nvec = sp_ceil(n_local, NV);
    s.cap = sp_max(p, 4096);
    s.blockB = f64 && n_local < kWide64Rows ? 64 : 32;
    s.cus = cus;
    s.step_grid = balanced_grid(sp_ceil(s.nvec, (int64_t)kSpBlock * kSpUnroll), sp_min(kMaxStepGrid, (int64_t)cus * kStepGridPerCU));
    s.block_grid = balanced_grid(sp_ceil(s.nvec, kSpBlock), (int64_t)cus * kBlockGridPerCU);
    s.gram_units = sp_ceil(s.nvec, (int64_t)kSpGramChunk * kSpGramWaves);
    // the widest record set of every user of the partials: k_step, k_blockstep, the column dots (pairs), and k_gramstep on the
    // larger of its two paths' grids
    int64_t d = (int64_t)kMaxStepGrid * kSpNSum;
    d = sp_max(d, (int64_t)cus * kBlockGridPerCU * sp_block_rec(kMaxBlockB));
    d = sp_max(d, kSpColBatch * kSpColChunks * 2);
    for (int NG = 4; NG >= 1; NG >>= 1)
        d = sp_max(d, (int64_t)cus * sp_max(gram_blocks_per_cu(NG, false), gram_blocks_per_cu(NG, true)) * sp_gram_rec(NG));
    s.partials_doubles = (size_t)d;
    return s;
}

// ---- the wide-block launch of one chunk (launch_gram_chunk) --------------------------------------------------------------------
enum GramVariant : int {
    kGramFrag = 0,      // k_gramstep<T, NG>: fragment loads, 64-vector chunks
    kGramLtLong = 1,    // k_gramstep<T, NG, true>: operands transposed through LDS, 64-vector chunks
    kGramLtShort = 2,   // k_gramstep<T, NG, true, 1>: ... chunks of one sub-chunk of 64 / NG vectors (NG >= 2)
};
struct GramPlan {
    GramVariant variant;
    int64_t cvn;       // chunk length in vectors
    int64_t nchunks;   // chunks over the nvec vectors (the last may be short)
    int grid;          // blocks: a wave takes chunks wave * grid + block, + kGramWaves * grid, ...
    int64_t rounds;    // trips of block 0's first wave (the most any wave makes)
};
// lt: CDH_LT (0 off, 1 on, 2 by size); ks: CDH_KS (0 by shard length, 1 short, 2 long).
// LDS-transposed (fully coalesced) operand loads: measured -5 % at >= 5e6 rows for every width; with short chunks also -10 %
// for B = 32 at 6.25e5 .. 1.25e6 rows and neutral for B = 64.  B = 16 takes it on long columns only.  fp32 B = 64 would spill
// (160 - 280 bytes per lane): fragment path, and its LDS-transposed variants are not instantiated.
constexpr GramPlan gram_plan(int64_t nvec, int64_t n, int cus, int NG, int esz, int lt, int ks) {
    const bool use_lt = (lt == 1 || (lt == 2 && (NG >= 2 || n >= kLtLongRows))) && !(NG == 4 && esz == 4);
    const int64_t gmax = (int64_t)cus * gram_blocks_per_cu(NG, use_lt);
    // short columns (a launch is fewer than kShortRounds rounds of 64-vector chunks on the grid those would get): chunks of one
    // sub-chunk, so a partly filled last round costs a quarter (B = 64) or half (B = 32) as much.  B = 16 has one sub-chunk
    // per chunk and a single LDS-transposed instantiation: long.
    const int G64 = balanced_grid(sp_ceil(nvec, (int64_t)kSpGramChunk * kSpGramWaves), gmax);
    const int64_t rounds64 = sp_ceil(nvec, kSpGramChunk) / ((int64_t)G64 * kSpGramWaves);
    const bool short_chunks = use_lt && NG >= 2 && (ks == 1 || (ks == 0 && rounds64 < kShortRounds));
    // ... and as many blocks as there are chunks of THAT length to hand out, four per block (the grid sized for 64-vector
    // chunks left 6 blocks to walk the 94 short chunks of a 24 KB column, four apiece and one after the other: 31 us per launch
    // whatever it read)
    const int64_t cvn = use_lt ? (int64_t)(kSpGramChunk / NG) * (short_chunks ? 1 : NG) : kSpGramChunk;
    const int64_t nchunks = sp_ceil(nvec, cvn);
    const int G = balanced_grid(sp_ceil(nchunks, kSpGramWaves), gmax);
    return GramPlan{!use_lt ? kGramFrag : short_chunks ? kGramLtShort : kGramLtLong, cvn, nchunks, G,
                    sp_ceil(nchunks, (int64_t)kSpGramWaves * G)};
}
// cdh_gram's read-only k_gramstep<T, 4> launch: the fragment path on the grid of its 64-vector chunks
constexpr int gram_read_grid(int64_t nvec, int cus) {
    return balanced_grid(sp_ceil(nvec, (int64_t)kSpGramChunk * kSpGramWaves), (int64_t)cus * gram_blocks_per_cu(4, false));
}

// ---- column dots over bc columns (col_dots, col_loadings; k_vc_expand splits its rows the same way: its sums are these sums) --
struct ColDotsPlan {
    int64_t groups;   // blocks across the columns, kColGroup each
    int chunks;       // row chunks: enough to fill the chip (~8 blocks per CU) but no more than kSpColChunks
    size_t doubles;   // partials written: `width` doubles per column of every group and chunk
};
constexpr ColDotsPlan col_dots_plan(int64_t bc, int64_t nvec, int cus, int width) {
    const int64_t groups = sp_ceil(bc, kSpColGroup);
    const int64_t want = sp_max(1, sp_ceil((int64_t)cus * kColFillPerCU, groups));
    const int chunks = (int)sp_max(1, sp_min(sp_min(kSpColChunks, want), sp_ceil(nvec, kSpBlock)));
    return ColDotsPlan{groups, chunks, (size_t)groups * chunks * width * kSpColGroup};
}

// ---- how a chunk of m visits runs (run_chunk) ------------------------------------------------------------------------------------
struct ChunkRoute {
    bool blocked;       // a launcher of blocks of B visits (false: launch_coord_chunk, a launch per visit)
    bool graph_worth;   // long enough for a captured graph to save anything
    uint64_t key;       // of its captured launch sequence
    int rewrites;       // launches that rewrite r: what ResidState::stream_enqueued is told
};
// block_mode: CDH_SWEEP_BLOCK; xbits: ExchangeState::graph_key_bits() (16 | 32).  Observation weights: the wide-block kernel
// carries them; the vector-ALU blocks (B <= 8) do not.  A graph of one or two launches saves nothing and costs a capture: short
// chunks go node by node.  The launch sequence of an m-visit chunk depends only on what the key holds.
constexpr ChunkRoute chunk_route(bool block_mode, int B, bool has_w, int m, unsigned xbits, bool dup) {
    const bool blocked = block_mode && (!has_w || B >= 16);
    const uint64_t key = ((uint64_t)m << 20) | ((uint64_t)(blocked ? B : 0) << 8) | xbits | (dup ? 4u : 0u) | (has_w ? 2u : 0u);
    return ChunkRoute{blocked, m >= (blocked ? 2 * B : 8), key, blocked ? (m + B - 1) / B + 1 : m + 1};
}

// ---- what a chunk counts towards cdh_profile_end: launches of its step kernel, and the bytes the algorithm has to move ------
// hs[0 .. m): the moves the visits made.  A visit reads its column and r (and w); a move is applied by the NEXT launch, which
// reads its column again and rewrites r; the last launch's moves by the trailing axpy.
// The chunk's terms are summed from zero, in the order they were once added to the running total one by one, and the caller adds
// the sum: every term is an integer number of bytes (n esz times a count), so up to 2^53 bytes -- 9 PB -- every partial sum is
// exact in a double and the total is the same bits whatever the grouping.
struct ChunkTraffic { int64_t launches; double bytes; };
constexpr ChunkTraffic chunk_traffic(bool blocked, int B, int m, bool has_w, const double* hs, int64_t n, size_t esz) {
    ChunkTraffic t{0, 0.0};
    const double vec = (double)n * (double)esz;
    if (!blocked) {
        t.launches += m;
        for (int i = 0; i < m; ++i) {
            const bool ap = i > 0 && hs[i - 1] != 0.0;
            t.bytes += vec * ((has_w ? 3.0 : 2.0) + (ap ? 2.0 : 0.0));
        }
        if (hs[m - 1] != 0.0) t.bytes += 3.0 * vec;
    } else {
        for (int pos0 = 0; pos0 < m; pos0 += B) {
            const int nb = m - pos0 < B ? m - pos0 : B;
            int nzp = 0;
            for (int i = pos0 - B > 0 ? pos0 - B : 0; i < pos0; ++i) nzp += hs[i] != 0.0;
            t.bytes += vec * (nb + 1 + nzp + (nzp ? 1 : 0));
            t.launches += 1;
        }
        int nzl = 0;
        for (int i = ((m - 1) / B) * B; i < m; ++i) nzl += hs[i] != 0.0;
        if (nzl) t.bytes += vec * (nzl + 2);
    }
    return t;
}
