// cox_score.hip -- the kernels of cdh_glm_cox_score: score and Schoenfeld residuals and the information matrix of a fitted Cox
// model with Breslow ties, for m <= kCoxScoreMaxCols chosen columns of the resident design (no reference counterpart: a round's
// solve is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194).  A translation unit of its own,
// linked into the same library: its kernels live in a FIFTH code object, and the four others -- first of all the one compiled
// from cdhip.hip, whose layout decides the flagship benchmark (cox_interval.hpp, LAB_NOTES) -- stay byte for byte what they were.
//
// The call runs AFTER the handle's own read-only step (cox_score_host.hpp), whose scratch holds, in sorted order, T (the
// stratum's suffix scan of ev = v e) and hA (the stratum's prefix scan of the hazard terms h = dv / S).  With xt = x - mu the
// centred column, everything new is the risk-set mean of a column, xbar = N / S at a tie group's first position, N the
// stratum's suffix scan of ev xt, and Q, the stratum's prefix scan of h xbar:
//   sch = xt - xbar                    at an event that counts (dv != 0 and S > 0: k_cox_hazard's rule), else exactly 0
//   L   = sch - e (xt A - Q)           A and Q read at the tie group's last position, e WITHOUT the weight
//   I   = sum ev A xt xt' - sum over the events that count of dv xbar xbar'
// The chain: the launches do not grow with m -- a column is blockIdx.y of a launch, or blockIdx.x of the one-workgroup scans of
// the runs' records -- and every column's numbers are formed by its own workgroups from its own scratch, so a column's sch and
// L are the same bits in any list.
//   k_score_centres, k_score_centres_sum   mu = the column's mean over the rows: 256 workgroups a column, their partials added
//                     in a fixed order (skipped when the caller gives centres)
//   k_score_prep      e, ev, h, dvk (dv at an event that counts) and wA = ev A by position: cox_eta's and k_cox_hazard's lines
//   k_score_gather    xt = X[order[s], c] - mu and ev xt in sorted order; the runs' records of the suffix scan by strata
//   k_score_offsets   the runs' records into exclusive offsets, one workgroup a column
//   k_score_scan      N
//   k_score_mean      h xbar at the events that count; the runs' records of the prefix scan by strata
//   k_score_offsets, k_score_scan    Q
//   k_score_rows      sch and L scattered through `order` to the caller's rows; pads are not written
//   k_score_info      the two sums of I per run in pair tiles of kCoxScorePair x kCoxScorePair columns (upper triangle of tiles)
//   k_score_info_sum  the runs' partials added in run order, ONE subtraction, the upper triangle mirrored
// The scans are the Cox step's (cox_kernels.hpp: a lane's four positions, the 64 lanes by shuffles, the four waves in order, the
// tiles of a run in order, the runs in order; the runs are cox_plan's, CDH_COX_GRID), written again here because that header is
// cdhip.hip's own.  They are always the segmented ones: a handle without strata has no head, and without a head the segmented
// scan is the plain scan addition for addition.  No atomics, no fences, no workgroup waits for another: every sum has one
// fixed order and every output is bit-identical run to run.  A product x_c x_d is formed before its factor, so I[c, d] and
// I[d, c] of any list are the same bits.
#include "cox_score.hpp"

#include "block_sum.hpp"

using namespace cdk;
static_assert(kCoxBlock == kBlock, "block_sum is block_sum.hpp's");
static_assert(kCoxPer == 4, "a lane holds four positions");
static_assert(kCoxMaxGrid == kCoxTile, "k_score_offsets scans the runs' records as one tile");
static_assert(kCoxScorePair == 4, "k_score_info holds a 4 x 4 pair tile per lane");

namespace {

constexpr int kPairVals = kCoxScorePair * kCoxScorePair;

// cox_block_excl<true>: the exclusive segmented scan of one (value, head seen) pair per lane over the workgroup, in lane order
__device__ __forceinline__ double score_block_excl(double v, double* s_w /* [kCoxBlock / 64] */, double& total, int& f,
                                                   int* s_f /* [kCoxBlock / 64] */, int& tf) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double x = v;
    int fl = f;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_up(x, d, 64);
        const int g = __shfl_up(fl, d, 64);
        if (lane >= d) {
            if (!fl) x = t + x;
            fl |= g;
        }
    }
    double ex = __shfl_up(x, 1, 64);
    int exf = __shfl_up(fl, 1, 64);
    if (lane == 0) { ex = 0.0; exf = 0; }
    __syncthreads();
    if (lane == 63) { s_w[wv] = x; s_f[wv] = fl; }
    __syncthreads();
    double base = 0.0, all = 0.0;
    int bf = 0, af = 0;
#pragma unroll
    for (int i = 0; i < kCoxBlock / 64; ++i) {
        const int g = s_f[i];
        if (i < wv) { base = g ? s_w[i] : base + s_w[i]; bf |= g; }
        all = g ? s_w[i] : all + s_w[i];
        af |= g;
    }
    total = all;
    tf = af;
    f = exf | bf;
    return exf ? ex : base + ex;
}

// k_cox_offsets<SUFFIX, true>: the records of `runs` runs into exclusive offsets, in place, one workgroup per column
// (blockIdx.x picks it, kCoxMaxGrid doubles apart; heads: one flag array for every column)
template <bool SUFFIX>
__global__ __launch_bounds__(kCoxBlock) void k_score_offsets(double* __restrict__ sums, int runs, const int32_t* __restrict__ heads) {
    __shared__ double s_w[kCoxBlock / 64];
    __shared__ int s_f[kCoxBlock / 64];
    double* v = sums + (int64_t)blockIdx.x * kCoxMaxGrid;
    const int q = SUFFIX ? kCoxBlock - 1 - (int)threadIdx.x : (int)threadIdx.x;
    double x[kCoxPer], l[kCoxPer];
    int hd[kCoxPer], fl[kCoxPer] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int i = q * kCoxPer + c;
        x[c] = i < runs ? v[i] : 0.0;
        hd[c] = i < runs ? heads[i] : 0;
    }
    double mine;
    int mf = 0;
    if (SUFFIX) {
        l[3] = 0.0;
        l[2] = x[3];                            fl[2] = hd[3];
        l[1] = hd[2] ? x[2] : l[2] + x[2];      fl[1] = fl[2] | hd[2];
        l[0] = hd[1] ? x[1] : l[1] + x[1];      fl[0] = fl[1] | hd[1];
        mine = hd[0] ? x[0] : l[0] + x[0];      mf = fl[0] | hd[0];
    } else {
        l[0] = 0.0;
        l[1] = x[0];                            fl[1] = hd[0];
        l[2] = hd[1] ? x[1] : l[1] + x[1];      fl[2] = fl[1] | hd[1];
        l[3] = hd[2] ? x[2] : l[2] + x[2];      fl[3] = fl[2] | hd[2];
        mine = hd[3] ? x[3] : l[3] + x[3];      mf = fl[3] | hd[3];
    }
    double total;
    int tf;
    const double base = score_block_excl(mine, s_w, total, mf, s_f, tf);
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int i = q * kCoxPer + c;
        if (i < runs) v[i] = fl[c] ? l[c] : base + l[c];
    }
}

// k_cox_scan<1, SUFFIX, true>: column blockIdx.y of v (ld apart; its offsets kCoxMaxGrid apart) becomes its inclusive suffix or
// prefix scan in place, restarting at every head bound[s] == s (bound == nullptr: no heads)
template <bool SUFFIX>
__global__ __launch_bounds__(kCoxBlock) void k_score_scan(double* __restrict__ v, const double* __restrict__ offs, int64_t ld,
                                                          int64_t tiles, const int32_t* __restrict__ bound) {
    __shared__ double s_w[kCoxBlock / 64];
    __shared__ int s_f[kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int q = SUFFIX ? kCoxBlock - 1 - (int)threadIdx.x : (int)threadIdx.x;
    double* va = v + (int64_t)blockIdx.y * ld;
    double carry = offs[(int64_t)blockIdx.y * kCoxMaxGrid + blockIdx.x];
    for (int64_t i = 0; i < t1 - t0; ++i) {
        const int64_t t = SUFFIX ? t1 - 1 - i : t0 + i;
        const int64_t s0 = t * kCoxTile + (int64_t)q * kCoxPer;
        const bool in = s0 < ld;              // (ld is a multiple of 32: a lane's positions lie wholly below ld or beyond)
        int hd[kCoxPer] = {0, 0, 0, 0};
        if (in && bound != nullptr) {
#pragma unroll
            for (int c = 0; c < kCoxPer; ++c) hd[c] = (int64_t)bound[s0 + c] == s0 + c;
        }
        double x[kCoxPer], l[kCoxPer];
        int fl[kCoxPer] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) x[c] = in ? va[s0 + c] : 0.0;
        if (SUFFIX) {
            l[3] = x[3];                            fl[3] = hd[3];
            l[2] = hd[2] ? x[2] : l[3] + x[2];      fl[2] = fl[3] | hd[2];
            l[1] = hd[1] ? x[1] : l[2] + x[1];      fl[1] = fl[2] | hd[1];
            l[0] = hd[0] ? x[0] : l[1] + x[0];      fl[0] = fl[1] | hd[0];
        } else {
            l[0] = x[0];                            fl[0] = hd[0];
            l[1] = hd[1] ? x[1] : l[0] + x[1];      fl[1] = fl[0] | hd[1];
            l[2] = hd[2] ? x[2] : l[1] + x[2];      fl[2] = fl[1] | hd[2];
            l[3] = hd[3] ? x[3] : l[2] + x[3];      fl[3] = fl[2] | hd[3];
        }
        double total;
        int f = SUFFIX ? fl[0] : fl[3], tf = 0;
        const double ex = score_block_excl(SUFFIX ? l[0] : l[3], s_w, total, f, s_f, tf);
        const double base = f ? ex : carry + ex;
        if (in) {
#pragma unroll
            for (int c = 0; c < kCoxPer; ++c) va[s0 + c] = fl[c] ? l[c] : base + l[c];
        }
        carry = tf ? total : carry + total;
    }
}

// The centres, in two launches.  Workgroup (g, c) adds column idx[c] over its share of the rows, g n / G .. (g + 1) n / G - 1 with
// G = kCoxScoreCentreRuns = gridDim.x: lane t the rows t, t + kCoxBlock, .. of the share in order, block_sum the lanes; the
// partial goes to part[c G + g] (the matrix's partials, written much later in the chain, lend their room).
__global__ __launch_bounds__(kCoxBlock) void k_score_centres(const double* __restrict__ X, int64_t ld, int64_t n,
                                                             const int32_t* __restrict__ idx, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double s_red[kCoxBlock / 64];
    const double* col = X + (int64_t)idx[blockIdx.y] * ld;
    const int64_t r0 = (int64_t)blockIdx.x * n / gridDim.x, r1 = (int64_t)(blockIdx.x + 1) * n / gridDim.x;
    double acc[1] = {0.0};
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kCoxBlock) acc[0] += col[i];
    block_sum<1>(acc, s_red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// mu[c] = the sum of column c's kCoxScoreCentreRuns partials, lane g holding partial g, in block_sum's fixed order, over n
__global__ __launch_bounds__(kCoxBlock) void k_score_centres_sum(const double* __restrict__ part, int64_t n, double* __restrict__ mu) {
#pragma clang fp contract(off)
    __shared__ double s_red[kCoxBlock / 64];
    double acc[1] = {part[(int64_t)blockIdx.x * kCoxScoreCentreRuns + threadIdx.x]};
    block_sum<1>(acc, s_red);
    if (threadIdx.x == 0) mu[blockIdx.x] = acc[0] / (double)n;
}
static_assert(kCoxScoreCentreRuns == kCoxBlock, "k_score_centres_sum: a lane a partial");

// Per sorted position: e = exp(min(eta, eta_max)) (cox_eta's lines), ev = v e and dv = v delta (k_cox_exp's products; pads: 0),
// S = T at the group's first position, the event counts when dv != 0 and S > 0 and then h = dv / S (k_cox_hazard's lines),
// dvk = dv at an event that counts, wA = ev A with A = hA at the group's last position.
__global__ __launch_bounds__(kCoxBlock) void k_score_prep(const int32_t* __restrict__ order, const int32_t* __restrict__ first,
                                                          const int32_t* __restrict__ last, const double* __restrict__ status,
                                                          const double* __restrict__ y, const double* __restrict__ r,
                                                          const double* __restrict__ offset, const double* __restrict__ weight,
                                                          int64_t n, int64_t ld, int64_t tiles, double eta_max,
                                                          const double* __restrict__ T, const double* __restrict__ hA,
                                                          double* __restrict__ e_out, double* __restrict__ ev_out,
                                                          double* __restrict__ h_out, double* __restrict__ dvk_out,
                                                          double* __restrict__ wA_out) {
#pragma clang fp contract(off)
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const int32_t row = order[s];
            const bool live = s < n;
            const double eta_lin = y[row] - r[row];
            const double eta = eta_lin + (offset != nullptr ? offset[row] : 0.0);
            const double ec = eta > eta_max ? eta_max : eta;
            const double e = exp(ec);
            double ev = e, dv = status[row];
            if (weight != nullptr) {
                const double v = weight[row];
                ev = v * e;
                dv = v * dv;
            }
            if (!live) { ev = 0.0; dv = 0.0; }
            const double S = T[first[s]];
            const bool haz = dv != 0.0 && S > 0.0;
            e_out[s] = e;
            ev_out[s] = ev;
            h_out[s] = haz ? dv / S : 0.0;
            dvk_out[s] = haz ? dv : 0.0;
            wA_out[s] = ev * hA[last[s]];
        }
    }
}

// Column blockIdx.y: xt = X[order[s], idx] - mu (pads: 0) and ev xt in sorted order, each operation rounded on its own; the
// run's record for the suffix scan by strata (k_cox_exp<true>'s): the sum over the run's positions up to the end of the stratum
// its first position lies in, head seen when that stratum ends inside the run.  slast == nullptr: one stratum, no head.
__global__ __launch_bounds__(kCoxBlock) void k_score_gather(const int32_t* __restrict__ order, const int32_t* __restrict__ slast,
                                                            const double* __restrict__ X, const int32_t* __restrict__ idx,
                                                            const double* __restrict__ mu, const double* __restrict__ ev,
                                                            int64_t n, int64_t ld, int64_t tiles, double* __restrict__ xt,
                                                            double* __restrict__ N, double* __restrict__ sums,
                                                            int32_t* __restrict__ heads) {
#pragma clang fp contract(off)
    __shared__ double s_red[kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int64_t bound = slast != nullptr ? (int64_t)slast[t0 * kCoxTile] : ld;
    const double* col = X + (int64_t)idx[blockIdx.y] * ld;
    const double centre = mu[blockIdx.y];
    double* xc = xt + (int64_t)blockIdx.y * ld;
    double* Nc = N + (int64_t)blockIdx.y * ld;
    double acc[1] = {0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const double x = s < n ? col[order[s]] - centre : 0.0;
            const double a = ev[s] * x;
            xc[s] = x;
            Nc[s] = a;
            acc[0] += s <= bound ? a : 0.0;
        }
    }
    block_sum<1>(acc, s_red);
    if (threadIdx.x == 0) {
        sums[(int64_t)blockIdx.y * kCoxMaxGrid + blockIdx.x] = acc[0];
        if (blockIdx.y == 0) {
            const int64_t end = t1 * kCoxTile < ld ? t1 * kCoxTile : ld;
            heads[blockIdx.x] = bound < end ? 1 : 0;
        }
    }
}

// Column blockIdx.y: h xbar at the events that count, xbar = N / S at the group's first position, else 0; the run's record
// for the prefix scan by strata (k_cox_hazard<true>'s): the sum over the run's positions from the start of the stratum its last
// position lies in, head seen when that stratum starts inside the run.  sfirst == nullptr: one stratum, no head.
__global__ __launch_bounds__(kCoxBlock) void k_score_mean(const int32_t* __restrict__ first, const int32_t* __restrict__ sfirst,
                                                          const double* __restrict__ T, const double* __restrict__ h,
                                                          const double* __restrict__ dvk, const double* __restrict__ N, int64_t ld,
                                                          int64_t tiles, double* __restrict__ Q, double* __restrict__ sums,
                                                          int32_t* __restrict__ heads) {
#pragma clang fp contract(off)
    __shared__ double s_red[kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int64_t end = t1 * kCoxTile < ld ? t1 * kCoxTile : ld;
    const int64_t bound = sfirst != nullptr ? (int64_t)sfirst[end - 1] : 0;
    const double* Nc = N + (int64_t)blockIdx.y * ld;
    double* Qc = Q + (int64_t)blockIdx.y * ld;
    double acc[1] = {0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            double a = 0.0;
            if (dvk[s] != 0.0) {
                const int32_t f = first[s];
                const double xbar = Nc[f] / T[f];
                a = h[s] * xbar;
            }
            Qc[s] = a;
            acc[0] += s >= bound ? a : 0.0;
        }
    }
    block_sum<1>(acc, s_red);
    if (threadIdx.x == 0) {
        sums[(int64_t)blockIdx.y * kCoxMaxGrid + blockIdx.x] = acc[0];
        if (blockIdx.y == 0) heads[blockIdx.x] = (sfirst != nullptr && bound >= t0 * kCoxTile) ? 1 : 0;
    }
}

// Column blockIdx.y, the rows: sch = xt - xbar at an event that counts, else 0; L = sch - e (xt A - Q), A and Q at the group's
// last position; scattered through `order`, column c at + c n.  Pads are not written; a nullptr output is skipped.
__global__ __launch_bounds__(kCoxBlock) void k_score_rows(const int32_t* __restrict__ order, const int32_t* __restrict__ first,
                                                          const int32_t* __restrict__ last, const double* __restrict__ T,
                                                          const double* __restrict__ hA, const double* __restrict__ e,
                                                          const double* __restrict__ dvk, const double* __restrict__ xt,
                                                          const double* __restrict__ N, const double* __restrict__ Q, int64_t n,
                                                          int64_t ld, int64_t tiles, double* __restrict__ sch_out,
                                                          double* __restrict__ score_out) {
#pragma clang fp contract(off)
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const double* xc = xt + (int64_t)blockIdx.y * ld;
    const double* Nc = N + (int64_t)blockIdx.y * ld;
    const double* Qc = Q + (int64_t)blockIdx.y * ld;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            if (s >= n) continue;
            const int32_t row = order[s];
            const double x = xc[s];
            double sch = 0.0;
            if (dvk[s] != 0.0) {
                const int32_t f = first[s];
                const double xbar = Nc[f] / T[f];
                sch = x - xbar;
            }
            if (sch_out != nullptr) sch_out[(int64_t)blockIdx.y * n + row] = sch;
            if (score_out != nullptr) {
                const int32_t l = last[s];
                const double xa = x * hA[l];
                const double d = xa - Qc[l];
                const double ed = e[s] * d;
                score_out[(int64_t)blockIdx.y * n + row] = sch - ed;
            }
        }
    }
}

// Pair tile blockIdx.y of the upper triangle of column tiles, run blockIdx.x: the run's share of
//   sum wA (xt_c xt_d)   and   sum over the events that count of dvk (xbar_c xbar_d)
// for the kCoxScorePair x kCoxScorePair pairs of the tile (a column at or beyond m stands as zeros), to
// part[((run pair_tiles + tile) 2 + which) kPairVals + i kCoxScorePair + j].
__global__ __launch_bounds__(kCoxBlock) void k_score_info(const int32_t* __restrict__ first, const double* __restrict__ T,
                                                          const double* __restrict__ wA, const double* __restrict__ dvk,
                                                          const double* __restrict__ xt, const double* __restrict__ N, int64_t n,
                                                          int64_t ld, int64_t tiles, int m, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double s_red[2 * kPairVals * (kCoxBlock / 64)];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const CoxScorePair pt = cox_score_pair(cox_score_col_tiles(m), blockIdx.y);
    const int c0 = (int)pt.ci * kCoxScorePair, d0 = (int)pt.di * kCoxScorePair;
    double acc[2 * kPairVals] = {};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            if (s >= n) continue;
            const double w = wA[s];
            double a[kCoxScorePair], b[kCoxScorePair];
#pragma unroll
            for (int i = 0; i < kCoxScorePair; ++i) {
                a[i] = c0 + i < m ? xt[(int64_t)(c0 + i) * ld + s] : 0.0;
                b[i] = d0 + i < m ? xt[(int64_t)(d0 + i) * ld + s] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < kCoxScorePair; ++i)
#pragma unroll
                for (int j = 0; j < kCoxScorePair; ++j) {
                    const double xx = a[i] * b[j];
                    acc[i * kCoxScorePair + j] += w * xx;
                }
            const double dk = dvk[s];
            if (dk != 0.0) {
                const int32_t f = first[s];
                const double S = T[f];
#pragma unroll
                for (int i = 0; i < kCoxScorePair; ++i) {
                    a[i] = c0 + i < m ? N[(int64_t)(c0 + i) * ld + f] / S : 0.0;
                    b[i] = d0 + i < m ? N[(int64_t)(d0 + i) * ld + f] / S : 0.0;
                }
#pragma unroll
                for (int i = 0; i < kCoxScorePair; ++i)
#pragma unroll
                    for (int j = 0; j < kCoxScorePair; ++j) {
                        const double xx = a[i] * b[j];
                        acc[kPairVals + i * kCoxScorePair + j] += dk * xx;
                    }
            }
        }
    }
    block_sum<2 * kPairVals>(acc, s_red);
    if (threadIdx.x == 0) {
        double* out = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 2 * kPairVals;
#pragma unroll
        for (int i = 0; i < 2 * kPairVals; ++i) out[i] = acc[i];
    }
}

// Pair tile blockIdx.x, lane = the pair inside it: the runs' partials added in run order, the second sum subtracted ONCE, and
// the entry written to info[c m + d] and info[d m + c] for c <= d < m (a diagonal tile's lower half is the mirror of its upper).
__global__ __launch_bounds__(64) void k_score_info_sum(const double* __restrict__ part, int runs, int m, double* __restrict__ info) {
#pragma clang fp contract(off)
    if (threadIdx.x >= kPairVals) return;
    const CoxScorePair pt = cox_score_pair(cox_score_col_tiles(m), blockIdx.x);
    const int c = (int)pt.ci * kCoxScorePair + (int)threadIdx.x / kCoxScorePair;
    const int d = (int)pt.di * kCoxScorePair + (int)threadIdx.x % kCoxScorePair;
    if (c >= m || d >= m || c > d) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < runs; ++b) {
        const double* p = part + ((int64_t)b * gridDim.x + blockIdx.x) * 2 * kPairVals;
        s1 += p[threadIdx.x];
        s2 += p[kPairVals + threadIdx.x];
    }
    const double v = s1 - s2;
    info[(int64_t)c * m + d] = v;
    info[(int64_t)d * m + c] = v;
}

}  // namespace

hipError_t cox_score_centres(hipStream_t stream, const CoxScoreIn& in, const CoxScoreBufs& b) {
    hipLaunchKernelGGL(k_score_centres, dim3((unsigned)kCoxScoreCentreRuns, (unsigned)in.m), dim3(kCoxBlock), 0, stream, in.X, in.ld,
                       in.n, (const int32_t*)b.idx, b.part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_centres_sum, dim3((unsigned)in.m), dim3(kCoxBlock), 0, stream, (const double*)b.part, in.n, b.mu);
    return hipGetLastError();
}

hipError_t cox_score_run(hipStream_t stream, const CoxPlan& pl, const CoxScoreIn& in, const CoxScoreBufs& b, bool want_sch,
                         bool want_score, bool want_info) {
    const dim3 runs((unsigned)pl.grid), cols((unsigned)pl.grid, (unsigned)in.m), percol((unsigned)in.m), block(kCoxBlock);
    hipError_t e;
    hipLaunchKernelGGL(k_score_prep, runs, block, 0, stream, in.order, in.first, in.last, in.status, in.y, in.r, in.offset,
                       in.weight, in.n, in.ld, pl.tiles, in.eta_max, in.T, in.hA, b.e, b.ev, b.h, b.dvk, b.wA);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_gather, cols, block, 0, stream, in.order, in.slast, in.X, (const int32_t*)b.idx,
                       (const double*)b.mu, (const double*)b.ev, in.n, in.ld, pl.tiles, b.xt, b.N, b.sums_N, b.heads_N);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_offsets<true>, percol, block, 0, stream, b.sums_N, (int)pl.grid, (const int32_t*)b.heads_N);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_scan<true>, cols, block, 0, stream, b.N, (const double*)b.sums_N, in.ld, pl.tiles, in.slast);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_mean, cols, block, 0, stream, in.first, in.sfirst, in.T, (const double*)b.h, (const double*)b.dvk,
                       (const double*)b.N, in.ld, pl.tiles, b.Q, b.sums_Q, b.heads_Q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_offsets<false>, percol, block, 0, stream, b.sums_Q, (int)pl.grid, (const int32_t*)b.heads_Q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_scan<false>, cols, block, 0, stream, b.Q, (const double*)b.sums_Q, in.ld, pl.tiles, in.sfirst);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (want_sch || want_score) {
        hipLaunchKernelGGL(k_score_rows, cols, block, 0, stream, in.order, in.first, in.last, in.T, in.hA, (const double*)b.e,
                           (const double*)b.dvk, (const double*)b.xt, (const double*)b.N, (const double*)b.Q, in.n, in.ld,
                           pl.tiles, want_sch ? b.sch : (double*)nullptr, want_score ? b.score : (double*)nullptr);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (want_info) {
        const unsigned pairs = (unsigned)cox_score_pair_tiles(in.m);
        hipLaunchKernelGGL(k_score_info, dim3((unsigned)pl.grid, pairs), block, 0, stream, in.first, in.T, (const double*)b.wA,
                           (const double*)b.dvk, (const double*)b.xt, (const double*)b.N, in.n, in.ld, pl.tiles, (int)in.m, b.part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_score_info_sum, dim3(pairs), dim3(64), 0, stream, (const double*)b.part, (int)pl.grid, (int)in.m,
                           b.info);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}
