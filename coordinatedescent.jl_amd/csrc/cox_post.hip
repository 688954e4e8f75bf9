// cox_post.hip -- the kernels of the Cox model's post-estimation exports (cdh_glm_cox_residuals, cdh_glm_cox_baseline; no
// reference counterpart: a round's solve is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194).  A
// translation unit of its own, linked into the same library: its kernels live in a THIRD code object, and the one compiled from
// cdhip.hip -- whose layout decides the flagship benchmark (cox_interval.hpp, LAB_NOTES) -- stays byte for byte what it was.
//
// Both exports run AFTER the handle's own read-only step (cox_post_host.hpp), whose scratch holds, in sorted order, T (and T2
// with start times), hA and hB -- the stratum's prefix scans of the hazard terms h and h2 -- and under Efron hc, the tie groups'
// scan of an event's own-group terms.  Nothing here adds a sum to a hazard: A of a row is READ from the step's scans.
//
// Both exports first build the table (five launches and two one-workgroup launches between them), and the rows read hA WHERE
// THE TABLE READS IT: at the last position of the last tie group at or before the row's that holds an event (post_at: the
// scanned flag at the row's group counts the table rows up to it, slotpos gives that row's position).  For a row whose own
// group holds an event that is last[s], the position its chain's apply kernel reads: the step's A bit for bit.  For a row in
// an event-free group the step reads hA further on, where the scan has added zeros only -- the same real number, but reached
// along another association of the same terms, so up to a few ulps away; read at the table's position instead, a row's cumhaz
// IS the table's step function at its time, == (and with start times the same one rounded subtraction of two table entries,
// exactly 0 where they are one entry).  An Efron event keeps its own expression.
//
// The rows (k_post_rows, one launch): per sorted position below n, e = exp(min(eta, eta_max)) WITHOUT the weight, A,
// M = delta - e A and the deviance residual sign(M) sqrt(-2 (M + delta log(e A))), scattered through `order` to the caller's
// rows.  Every operation is rounded on its own.
//
// The table: one row per tie group below n that holds an event,
//   k_post_mark      dv = v delta in sorted order and the runs' records of its scan by TIE GROUP (heads: first[s] == s)
//   k_post_offsets   the runs' records into exclusive offsets
//   k_post_scan      dv prefix-scanned inside the tie group: at the group's last position, n_event
//   k_post_flag      flag = 1 at the last position of a group with n_event > 0, else 0; the runs' counts
//   k_post_offsets   the runs' counts into exclusive offsets, their total: the table's length
//   k_post_scan      the flags prefix-scanned (plain): a flagged position's slot is its scan less one
//   k_post_scatter   the six columns to the slot, and the group's last position to slotpos[slot]
// The scans are the Cox step's (cox_kernels.hpp: a lane's four positions, the 64 lanes by shuffles, the four waves in order, the
// tiles of a run in order, the runs in order), written again here because that header is cdhip.hip's own: every sum has one
// fixed order and the table's order is the sort's, so both exports are bit-identical run to run.  The flags are doubles: their
// sums are integers far below 2^53, exact in any order, and the one scan serves both.  The runs are cox_plan's (CDH_COX_GRID).
#include "cox_post.hpp"

#include "block_sum.hpp"

using namespace cdk;
static_assert(kCoxBlock == kBlock, "block_sum is block_sum.hpp's");
static_assert(kCoxPer == 4, "a lane holds four positions");
static_assert(kCoxMaxGrid == kCoxTile, "k_post_offsets scans the runs' records as one tile");

namespace {

// The exclusive segmented prefix scan of one (value, head seen) pair per lane over the workgroup, under
// (f1, v1) + (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2): -> the sum since the last head among the lanes before this one; f becomes
// whether there is one; total and tf: the workgroup's pair.  Without a head it is the plain scan, addition for addition.
__device__ __forceinline__ double post_block_excl(double v, int& f, double& total, int& tf, double* s_w /* [kCoxBlock / 64] */,
                                                  int* s_f /* [kCoxBlock / 64] */) {
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
    __syncthreads();                          // (the previous trip's readers of s_w are done)
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

// a lane's four values into inclusive scans since the last head at or before each (l, fl); hd: the heads
__device__ __forceinline__ void post_lane_scan(const double (&x)[kCoxPer], const int (&hd)[kCoxPer], double (&l)[kCoxPer],
                                               int (&fl)[kCoxPer]) {
    l[0] = x[0];                            fl[0] = hd[0];
    l[1] = hd[1] ? x[1] : l[0] + x[1];      fl[1] = fl[0] | hd[1];
    l[2] = hd[2] ? x[2] : l[1] + x[2];      fl[2] = fl[1] | hd[2];
    l[3] = hd[3] ? x[3] : l[2] + x[3];      fl[3] = fl[2] | hd[3];
}

// The runs' records (sum since the last head, head seen: heads[i]; heads == nullptr: no heads) into exclusive offsets, in
// place, by one workgroup; a lane holds kCoxPer runs.  total != nullptr: the sum of all the records (a plain scan's only).
__global__ __launch_bounds__(kCoxBlock) void k_post_offsets(double* __restrict__ sums, int runs, const int32_t* __restrict__ heads,
                                                            double* __restrict__ total) {
    __shared__ double s_w[kCoxBlock / 64];
    __shared__ int s_f[kCoxBlock / 64];
    double x[kCoxPer], l[kCoxPer];
    int hd[kCoxPer], fl[kCoxPer];
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int i = (int)threadIdx.x * kCoxPer + c;
        x[c] = i < runs ? sums[i] : 0.0;
        hd[c] = (heads != nullptr && i < runs) ? heads[i] : 0;
    }
    post_lane_scan(x, hd, l, fl);
    double all;
    int f = fl[3], tf;
    const double ex = post_block_excl(l[3], f, all, tf, s_w, s_f);
    // exclusive: what came before position c -- the lane's base, then the lane's own values before c
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int i = (int)threadIdx.x * kCoxPer + c;
        if (i < runs) sums[i] = c == 0 ? ex : (fl[c - 1] ? l[c - 1] : ex + l[c - 1]);
    }
    if (total != nullptr && threadIdx.x == 0) *total = all;
}

// v becomes its inclusive prefix scan in place, restarting at every head bound[s] == s (bound == nullptr: a plain scan);
// workgroup b walks its run forwards and carries the sum since the last head from tile to tile, starting at its run's offset.
__global__ __launch_bounds__(kCoxBlock) void k_post_scan(double* __restrict__ v, const double* __restrict__ offs, int64_t ld,
                                                         int64_t tiles, const int32_t* __restrict__ bound) {
    __shared__ double s_w[kCoxBlock / 64];
    __shared__ int s_f[kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    double carry = offs[blockIdx.x];
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        const bool in = s0 < ld;              // (ld is a multiple of 32: a lane's positions lie wholly below ld or beyond)
        double x[kCoxPer], l[kCoxPer];
        int hd[kCoxPer], fl[kCoxPer];
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            x[c] = in ? v[s0 + c] : 0.0;
            hd[c] = (in && bound != nullptr) ? (int64_t)bound[s0 + c] == s0 + c : 0;
        }
        post_lane_scan(x, hd, l, fl);
        double total;
        int f = fl[3], tf;
        const double ex = post_block_excl(l[3], f, total, tf, s_w, s_f);
        const double base = f ? ex : carry + ex;
        if (in) {
#pragma unroll
            for (int c = 0; c < kCoxPer; ++c) v[s0 + c] = fl[c] ? l[c] : base + l[c];
        }
        carry = tf ? total : carry + total;
    }
}

// dv = v delta of the row at every sorted position (pads: 0), the product rounded on its own as in k_cox_exp; the run's record
// for the scan by tie group: the sum over the run's positions from the first position of the group its last position lies
// in, head seen when that group starts inside the run (k_efron_mark's record).
__global__ __launch_bounds__(kCoxBlock) void k_post_mark(const int32_t* __restrict__ order, const int32_t* __restrict__ first,
                                                         const double* __restrict__ status, const double* __restrict__ weight,
                                                         int64_t n, int64_t ld, int64_t tiles, double* __restrict__ dv,
                                                         double* __restrict__ sums, int32_t* __restrict__ heads) {
#pragma clang fp contract(off)
    __shared__ double s_red[kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int64_t end = t1 * kCoxTile < ld ? t1 * kCoxTile : ld;
    const int64_t gb = first[end - 1];
    double acc[1] = {0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const int32_t row = order[s];
            const double d = s < n ? (weight != nullptr ? weight[row] * status[row] : status[row]) : 0.0;
            dv[s] = d;
            acc[0] += s >= gb ? d : 0.0;
        }
    }
    block_sum<1>(acc, s_red);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = acc[0];
        heads[blockIdx.x] = gb >= t0 * kCoxTile ? 1 : 0;
    }
}

// is sorted position s the last of a tie group below n that holds an event?  dv: scanned inside the tie group
__device__ __forceinline__ bool post_flagged(const int32_t* __restrict__ last, const double* __restrict__ dv, int64_t n, int64_t s) {
    return s < n && (int64_t)last[s] == s && dv[s] > 0.0;
}

// the flags and their number per run
__global__ __launch_bounds__(kCoxBlock) void k_post_flag(const int32_t* __restrict__ last, const double* __restrict__ dv, int64_t n,
                                                         int64_t ld, int64_t tiles, double* __restrict__ flag,
                                                         double* __restrict__ sums) {
    __shared__ double s_red[kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    double acc[1] = {0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const double f = post_flagged(last, dv, n, s0 + c) ? 1.0 : 0.0;
            flag[s0 + c] = f;
            acc[0] += f;
        }
    }
    block_sum<1>(acc, s_red);
    if (threadIdx.x == 0) sums[blockIdx.x] = acc[0];
}

// a[at] - (sub >= 0 ? b[sub] : 0): cox_interval.hpp's cox_less, the one rounded subtraction of the interval chain
__device__ __forceinline__ double post_less(const double* a, int32_t at, const double* b, int32_t sub) {
#pragma clang fp contract(off)
    return a[at] - (sub >= 0 ? b[sub] : 0.0);
}

// A flagged position writes its group's row to slot flag[s] - 1: the slots are 0 .. count - 1 in sorted order, each written by
// the one lane that holds the group's last position; count <= n <= ld, and a slot outside 0 .. ld - 1 is not written.
__global__ __launch_bounds__(kCoxBlock) void k_post_scatter(const int32_t* __restrict__ order, const int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ last, const int32_t* __restrict__ lo,
                                                            const double* __restrict__ time, const int32_t* __restrict__ strata,
                                                            const double* __restrict__ dv, const double* __restrict__ flag,
                                                            const double* __restrict__ eT, const double* __restrict__ T2,
                                                            const double* __restrict__ hA, const double* __restrict__ hB, int64_t n,
                                                            int64_t ld, int64_t tiles, double* __restrict__ out,
                                                            int32_t* __restrict__ stratum, int32_t* __restrict__ slotpos) {
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            if (!post_flagged(last, dv, n, s)) continue;
            const int64_t slot = (int64_t)flag[s] - 1;
            if (slot < 0 || slot >= ld) continue;
            const int32_t row = order[s];
            slotpos[slot] = (int32_t)s;
            stratum[slot] = strata != nullptr ? strata[row] : 0;
            out[slot] = time[row];
            out[ld + slot] = dv[s];
            out[2 * ld + slot] = lo != nullptr ? post_less(eT, first[s], T2, lo[s]) : eT[first[s]];
            out[3 * ld + slot] = hA[s];
            out[4 * ld + slot] = hB[s];
        }
    }
}

// The last position of the last tie group that the table holds among those ending at or before position x (a group's last
// position, or -1), inside the stratum that starts at sf; -1: none.  flag: scanned, so flag[x] counts those groups over ALL
// strata, and slotpos of the last of them lies in front of sf when the stratum has none.  flag[x] <= the table's length <= n.
__device__ __forceinline__ int32_t post_at(const double* __restrict__ flag, const int32_t* __restrict__ slotpos, int32_t x,
                                           int32_t sf) {
    if (x < 0) return -1;
    const int64_t c = (int64_t)flag[x];
    if (c <= 0) return -1;
    const int32_t p = slotpos[c - 1];
    return p >= sf ? p : -1;
}

// The rows' export, after the table's launches.  eta, its cap and e are cox_eta's lines; A is hA read at the table's positions
// (the head of this file), for an Efron event the chain's own expression (CHAIN, chosen on the host); pads are not written.
// The deviance residual's radicand -2 (M + delta log(e A)) is >= 0 in exact arithmetic and can round below zero only where
// e A is within rounding of 1: there it is taken as 0, where plain IEEE arithmetic (and R's residuals.coxph) would give NaN.
// An event with e A = 0 (its own term was skipped) gives log 0 = -inf and the residual +inf.
template <CoxPostChain CHAIN>
__global__ __launch_bounds__(kCoxBlock) void k_post_rows(const int32_t* __restrict__ order, const int32_t* __restrict__ first,
                                                         const int32_t* __restrict__ last, const int32_t* __restrict__ sfirst,
                                                         const int32_t* __restrict__ enter, const double* __restrict__ status,
                                                         const double* __restrict__ y, const double* __restrict__ r,
                                                         const double* __restrict__ offset, int64_t n, int64_t ld, int64_t tiles,
                                                         double eta_max, const double* __restrict__ hA,
                                                         const double* __restrict__ hc, const double* __restrict__ flag,
                                                         const int32_t* __restrict__ slotpos, double* __restrict__ cumhaz,
                                                         double* __restrict__ martingale, double* __restrict__ deviance) {
#pragma clang fp contract(off)
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            if (s >= n) continue;
            const int32_t row = order[s];
            const double eta_lin = y[row] - r[row];
            const double eta = eta_lin + (offset != nullptr ? offset[row] : 0.0);
            const double ec = eta > eta_max ? eta_max : eta;
            const double e = exp(ec);
            const double delta = status[row];
            const int32_t l = last[s];
            const int32_t sf = sfirst != nullptr ? sfirst[s] : 0;
            const int32_t at = post_at(flag, slotpos, l, sf);
            double A = at >= 0 ? hA[at] : 0.0;
            if constexpr (CHAIN == CoxPostChain::Interval) {
                if (at >= 0) A = post_less(hA, at, hA, post_at(flag, slotpos, enter[s], sf));
            }
            if constexpr (CHAIN == CoxPostChain::Efron) {
                if (delta != 0.0) {
                    const int32_t f = first[s];
                    A = (f > sf ? hA[f - 1] : 0.0) + hc[l];
                }
            }
            const double eA = e * A;
            const double M = delta - eA;
            if (cumhaz != nullptr) cumhaz[row] = A;
            if (martingale != nullptr) martingale[row] = M;
            if (deviance != nullptr) {
                const double lg = delta != 0.0 ? delta * log(eA) : 0.0;
                const double rad = -2.0 * (M + lg);
                const double root = sqrt(rad < 0.0 ? 0.0 : rad);
                deviance[row] = M > 0.0 ? root : (M < 0.0 ? -root : 0.0);
            }
        }
    }
}

}  // namespace

hipError_t cox_post_rows(hipStream_t stream, const CoxPlan& pl, CoxPostChain chain, const CoxPostIn& in, const CoxPostBufs& b,
                         const bool want[3]) {
    double* cum = want[0] ? b.out : nullptr;
    double* mart = want[1] ? b.out + in.ld : nullptr;
    double* dev = want[2] ? b.out + 2 * in.ld : nullptr;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid), dim3(kCoxBlock), 0, stream, in.order, in.first, in.last, in.sfirst,
                           in.enter, in.status, in.y, in.r, in.offset, in.n, in.ld, pl.tiles, in.eta_max, in.hA, in.hc,
                           (const double*)b.flag, (const int32_t*)b.slotpos, cum, mart, dev);
    };
    if (chain == CoxPostChain::Efron) go(k_post_rows<CoxPostChain::Efron>);
    else if (chain == CoxPostChain::Interval) go(k_post_rows<CoxPostChain::Interval>);
    else go(k_post_rows<CoxPostChain::Censored>);
    return hipGetLastError();
}

hipError_t cox_post_table(hipStream_t stream, const CoxPlan& pl, const CoxPostIn& in, const CoxPostBufs& b) {
    const dim3 grid((unsigned)pl.grid), one(1), block(kCoxBlock);
    double *sums_dv = b.sums, *sums_flag = b.sums + kCoxMaxGrid;
    hipError_t e;
    hipLaunchKernelGGL(k_post_mark, grid, block, 0, stream, in.order, in.first, in.status, in.weight, in.n, in.ld, pl.tiles, b.dv,
                       sums_dv, b.heads);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_post_offsets, one, block, 0, stream, sums_dv, (int)pl.grid, (const int32_t*)b.heads, (double*)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_post_scan, grid, block, 0, stream, b.dv, (const double*)sums_dv, in.ld, pl.tiles, in.first);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_post_flag, grid, block, 0, stream, in.last, (const double*)b.dv, in.n, in.ld, pl.tiles, b.flag, sums_flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_post_offsets, one, block, 0, stream, sums_flag, (int)pl.grid, (const int32_t*)nullptr, b.total);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_post_scan, grid, block, 0, stream, b.flag, (const double*)sums_flag, in.ld, pl.tiles,
                       (const int32_t*)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_post_scatter, grid, block, 0, stream, in.order, in.first, in.last, in.lo, in.time, in.strata,
                       (const double*)b.dv, (const double*)b.flag, in.eT, in.T2, in.hA, in.hB, in.n, in.ld, pl.tiles, b.out,
                       b.stratum, b.slotpos);
    return hipGetLastError();
}
