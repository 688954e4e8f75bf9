// cox_concordance.hip -- the kernels of Harrell's concordance index of a Cox model (cdh_glm_cox_concordance; no reference
// counterpart: a round's solve is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194).  A translation
// unit of its own, linked into the same library: its kernels live in a FOURTH code object, and the one compiled from cdhip.hip
// -- whose layout decides the flagship benchmark (cox_interval.hpp, LAB_NOTES) -- stays what it was.
//
// C asks of every event row how many of the rows that outlive it have a smaller, an equal or a larger eta.  In the concordance
// order (cox_plan.hpp: cox_conc_order) those rows are one range of positions [qa, qb), so the question is a two-dimensional
// dominance count, answered by a merge sort of eta over the positions with the counts read off its levels: at level lev the
// positions are cut into runs of 2^lev, each sorted by eta, and a range is at most two whole runs per level (cox_conc_take).
// In a run the weight of the smaller eta is the run's prefix sum of the weights at the event's lower-bound rank, that of the
// smaller-or-equal eta the prefix sum at its upper-bound rank, and the run's total its last prefix sum.  Rows outside the subset
// and pads carry the key +inf and the weight 0; a handle without weights carries the weight 1, whose sums are exact integers.
//
//   k_conc_tile     eta of the row at every position (cox_eta's two lines, NOT capped), the subset mask from the fold ids, the NaN
//                   count of the tile; the tile's positions sorted level by level in LDS, levels 0 .. kCoxTileLog - 1, and the
//                   sorted tile -- level kCoxTileLog -- written out with its prefix sums
//   k_conc_fringe   the two fringes of every event's range (cox_conc_fringe: what the walk takes of the levels below the tile),
//                   counted position by position in ascending order: the rows' sums L, E, G start here
//   k_conc_level    once per level from the tile's to the one below the top: every event's at most two runs of this level, added
//                   to L, E, G; then (all but the last) the next level by merge-path ranks into the other pair of the ping-pong
//   k_conc_rows     v L, v (E - L), v (G - E) of every position, summed per tile (block_sum)
//   k_conc_total    the tiles' records added in tile order by one workgroup
//
// The prefix sums need no scan.  An element that moves to rank i + j of the merged run -- i its rank in its own run, j the
// number of the sibling run's elements that go before it -- has the inclusive prefix sum P_own[i] + P_sibling[j - 1]: ONE
// rounded addition per level, of two sums over disjoint rows, so a prefix sum at level lev carries at most lev roundings.
// Equal keys are ordered left run first (lower bound for the left run's elements, upper bound for the right's); the ranks
// read off a run fall on the edges of its groups of equal keys, where that order does not matter.
//
// Every sum has one fixed order -- a fringe by ascending position, the levels ascending, at a level the left run before the
// right, the tiles in order -- so the four numbers are bit-identical run to run.
#include "cox_concordance.hpp"

#include "block_sum.hpp"

using namespace cdk;
static_assert(kCoxBlock == kBlock, "block_sum is block_sum.hpp's");
static_assert(kCoxPer == 4 && kCoxTile == (int64_t)kCoxBlock * kCoxPer, "a lane holds four positions of a tile");

namespace {

constexpr int kTile = (int)kCoxTile;

// the number of k[0 .. len) that are < x (lower bound) and <= x (upper bound); k ascending
__device__ __forceinline__ int64_t conc_lower(const double* __restrict__ k, int64_t len, double x) {
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (k[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int64_t conc_upper(const double* __restrict__ k, int64_t len, double x) {
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (k[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Lane t holds the tile's positions t, t + 256, t + 512, t + 768 (coalesced).  ka, pa: the sorted tile and its prefix sums.
// part[4 tile + 3]: the tile's NaN count.
__global__ __launch_bounds__(kCoxBlock) void k_conc_tile(const int32_t* __restrict__ order, const double* __restrict__ y,
                                                         const double* __restrict__ r, const double* __restrict__ offset,
                                                         const double* __restrict__ weight, const uint8_t* __restrict__ fold, int k,
                                                         int64_t n, double* __restrict__ key0, double* __restrict__ v0,
                                                         double* __restrict__ ka, double* __restrict__ pa, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double s_k[2][kTile];
    __shared__ double s_p[2][kTile];
    __shared__ double s_red[kCoxBlock / 64];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    double bad[1] = {0.0};
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int e = c * kCoxBlock + (int)threadIdx.x;
        const int64_t p = base + e;
        double key = __builtin_inf(), v = 0.0;
        if (p < n) {
            const int32_t row = order[p];
            if (fold == nullptr || (int)fold[row] == k) {
                const double eta_lin = y[row] - r[row];
                const double eta = eta_lin + (offset != nullptr ? offset[row] : 0.0);
                if (eta != eta) bad[0] += 1.0;
                else { key = eta; v = weight != nullptr ? weight[row] : 1.0; }
            }
        }
        key0[p] = key;
        v0[p] = v;
        s_k[0][e] = key;
        s_p[0][e] = v;
    }
    __syncthreads();
    int src = 0;
    for (int lev = 0; lev < kCoxTileLog; ++lev) {
        const int len = 1 << lev;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int e = c * kCoxBlock + (int)threadIdx.x;
            const int m = e >> lev, own = m << lev, sib = (m ^ 1) << lev;
            const double key = s_k[src][e];
            const int j = (int)((m & 1) ? conc_upper(&s_k[src][sib], len, key) : conc_lower(&s_k[src][sib], len, key));
            const int pos = ((m & ~1) << lev) + (e - own) + j;
            s_k[src ^ 1][pos] = key;
            s_p[src ^ 1][pos] = j > 0 ? s_p[src][e] + s_p[src][sib + j - 1] : s_p[src][e];
        }
        __syncthreads();
        src ^= 1;
    }
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int e = c * kCoxBlock + (int)threadIdx.x;
        ka[base + e] = s_k[src][e];
        pa[base + e] = s_p[src][e];
    }
    block_sum<1>(bad, s_red);
    if (threadIdx.x == 0) part[4 * (int64_t)blockIdx.x + 3] = bad[0];
}

// does position p hold an event that takes part?  (a row that takes part has a weight > 0; qa < qb marks the events)
__device__ __forceinline__ bool conc_asks(const double* __restrict__ v0, const int32_t* __restrict__ qa,
                                          const int32_t* __restrict__ qb, int64_t p) {
    return v0[p] > 0.0 && qa[p] < qb[p];
}

// L, E, G of every position: the two fringes of its range, [a, a1) then [b0, b), each by ascending position (a term that
// does not count adds 0.0, which changes nothing); 0 where nothing is asked
__global__ __launch_bounds__(kCoxBlock) void k_conc_fringe(const double* __restrict__ key0, const double* __restrict__ v0,
                                                           const int32_t* __restrict__ qa, const int32_t* __restrict__ qb,
                                                           double* __restrict__ L, double* __restrict__ E, double* __restrict__ G) {
#pragma clang fp contract(off)
    const int64_t base = (int64_t)blockIdx.x * kTile;
#pragma unroll 1
    for (int c = 0; c < kCoxPer; ++c) {
        const int64_t p = base + c * kCoxBlock + (int64_t)threadIdx.x;
        double l = 0.0, e = 0.0, g = 0.0;
        if (conc_asks(v0, qa, qb, p)) {
            const double x = key0[p];
            const int64_t a = qa[p], b = qb[p];
            const CoxConcFringe f = cox_conc_fringe(a, b);
            for (int64_t j = a; j < f.a1; ++j) {
                const double kj = key0[j], vj = v0[j];
                l += kj < x ? vj : 0.0;
                e += kj <= x ? vj : 0.0;
                g += vj;
            }
            for (int64_t j = f.b0; j < b; ++j) {
                const double kj = key0[j], vj = v0[j];
                l += kj < x ? vj : 0.0;
                e += kj <= x ? vj : 0.0;
                g += vj;
            }
        }
        L[p] = l;
        E[p] = e;
        G[p] = g;
    }
}

// Level lev >= kCoxTileLog in (kin, pin), N positions (a multiple of the tile, so every run is whole tiles and only the last
// run of a level can be short or, for an even run, lack its sibling).  The runs an event takes are whole runs below n <= N.
__global__ __launch_bounds__(kCoxBlock) void k_conc_level(const double* __restrict__ kin, const double* __restrict__ pin,
                                                          double* __restrict__ kout, double* __restrict__ pout,
                                                          const double* __restrict__ key0, const double* __restrict__ v0,
                                                          const int32_t* __restrict__ qa, const int32_t* __restrict__ qb, int64_t N,
                                                          int lev, int merge, double* __restrict__ L, double* __restrict__ E,
                                                          double* __restrict__ G) {
#pragma clang fp contract(off)
    const int64_t base = (int64_t)blockIdx.x * kTile, len = (int64_t)1 << lev;
#pragma unroll 1
    for (int c = 0; c < kCoxPer; ++c) {
        const int64_t p = base + c * kCoxBlock + (int64_t)threadIdx.x;
        if (conc_asks(v0, qa, qb, p)) {
            const CoxConcTake t = cox_conc_take(qa[p], qb[p], lev);
            if (t.count > 0) {
                const double x = key0[p];
                double l = L[p], e = E[p], g = G[p];
                for (int i = 0; i < t.count; ++i) {
                    const int64_t rb = t.run[i] << lev;
                    const int64_t lo = conc_lower(kin + rb, len, x), up = conc_upper(kin + rb, len, x);
                    l += lo > 0 ? pin[rb + lo - 1] : 0.0;
                    e += up > 0 ? pin[rb + up - 1] : 0.0;
                    g += pin[rb + len - 1];
                }
                L[p] = l;
                E[p] = e;
                G[p] = g;
            }
        }
        if (merge) {
            const int64_t m = p >> lev, own = m << lev, sib = (m ^ 1) << lev;
            const double key = kin[p], pre = pin[p];
            if (sib >= N) {                   // an even last run without a sibling moves up as it is
                kout[p] = key;
                pout[p] = pre;
            } else {
                const int64_t sl = N - sib < len ? N - sib : len;
                const int64_t j = (m & 1) ? conc_upper(kin + sib, sl, key) : conc_lower(kin + sib, sl, key);
                const int64_t pos = ((m & ~(int64_t)1) << lev) + (p - own) + j;
                kout[pos] = key;
                pout[pos] = j > 0 ? pre + pin[sib + j - 1] : pre;
            }
        }
    }
}

// an event's three products, every operation rounded on its own; the tile's sums into part[4 tile + 0 .. 2]
__global__ __launch_bounds__(kCoxBlock) void k_conc_rows(const double* __restrict__ v0, const int32_t* __restrict__ qa,
                                                         const int32_t* __restrict__ qb, const double* __restrict__ L,
                                                         const double* __restrict__ E, const double* __restrict__ G,
                                                         double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double s_red[3 * (kCoxBlock / 64)];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int64_t p = base + c * kCoxBlock + (int64_t)threadIdx.x;
        if (!conc_asks(v0, qa, qb, p)) continue;
        const double v = v0[p], l = L[p], e = E[p], g = G[p];
        const double tied = e - l, above = g - e;
        acc[0] += v * l;
        acc[1] += v * above;
        acc[2] += v * tied;
    }
    block_sum<3>(acc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) part[4 * (int64_t)blockIdx.x + i] = acc[i];
    }
}

// the tiles' records added in tile order: lane t takes tiles t, t + 256, .., then the workgroup's sum
__global__ __launch_bounds__(kCoxBlock) void k_conc_total(const double* __restrict__ part, int64_t tiles, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_red[4 * (kCoxBlock / 64)];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = threadIdx.x; t < tiles; t += kCoxBlock) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += part[4 * t + i];
    }
    block_sum<4>(acc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = acc[i];
    }
}

}  // namespace

hipError_t cox_conc_run(hipStream_t stream, const CoxConcIn& in, const CoxConcBufs& b) {
    const dim3 grid((unsigned)b.tiles), one(1), block(kCoxBlock);
    hipError_t e;
    hipLaunchKernelGGL(k_conc_tile, grid, block, 0, stream, b.order, in.y, in.r, in.offset, in.weight, in.fold, (int)in.k, in.n,
                       b.key0, b.v0, b.ka, b.pa, b.part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_conc_fringe, grid, block, 0, stream, (const double*)b.key0, (const double*)b.v0, b.qa, b.qb, b.L, b.E, b.G);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // The one run of level top is never taken: it would need qa == 0, and qa[s] > s.  So the last level queried is top - 1
    // (taken only when n == N == 2^top), and the last one merged INTO: the merges run at the levels below it.
    const int top = cox_conc_top(b.N);
    double *kin = b.ka, *pin = b.pa, *kout = b.kb, *pout = b.pb;
    for (int lev = kCoxTileLog; lev < top; ++lev) {
        hipLaunchKernelGGL(k_conc_level, grid, block, 0, stream, (const double*)kin, (const double*)pin, kout, pout,
                           (const double*)b.key0, (const double*)b.v0, b.qa, b.qb, b.N, lev, lev < top - 1 ? 1 : 0, b.L, b.E, b.G);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        std::swap(kin, kout);
        std::swap(pin, pout);
    }
    hipLaunchKernelGGL(k_conc_rows, grid, block, 0, stream, (const double*)b.v0, b.qa, b.qb, (const double*)b.L, (const double*)b.E,
                       (const double*)b.G, b.part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_conc_total, one, block, 0, stream, (const double*)b.part, b.tiles, b.out);
    return hipGetLastError();
}
