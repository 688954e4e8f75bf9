// cox_efron.hip -- the three kernels the Cox step adds for Efron ties (cdh_glm_set_cox_ties; no reference counterpart: a
// round's solve is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194).  A translation unit of its
// own, linked into the same library: its kernels live in a SECOND code object, and the one compiled from cdhip.hip -- whose
// layout decides the flagship benchmark (cox_interval.hpp, LAB_NOTES) -- stays byte for byte what it was.
//
// The mathematics (survival::coxph's ties = "efron", its convention for weights).  Per training row ev = v e and dv = v delta;
// everything inside the row's stratum.  A tie group g -- a run first .. last of sorted positions with one time -- has among
// its TRAINING rows d events, D = sum of ev over them, m = (sum of dv over them) / d and the risk-set sum S = T[first].  Its
// events are numbered l = 0 .. d - 1 in sorted order, den_l = S - (l / d) D, and
//   n nll = sum_g [ m sum_l log den_l - sum over the events of g of dv eta ]
//   A_i   = sum over the groups g at or before i's of m sum_l c / den_l,     B_i likewise with c^2 / den_l^2,
// where c = 1 - l / d if i is an event of g itself and c = 1 otherwise.  d = 1 gives Breslow: m = dv, den = S.
//
// No loop over a group, no atomics: every event position holds its own l, and sums over a group are scans that restart at the
// group's bounds -- k_cox_scan<., ., true> of cox_kernels.hpp with `first` or `last` as its heads.  The chain, launched by
// cox_launch_efron (cox_efron_host.hpp), always segmented and weighted like the interval chain:
//   k_cox_exp<true>     ev and dv in sorted order, as today
//   k_efron_mark        cnt = [event], Dv = ev [event], Sdv = dv, while eT still holds ev; their runs' records
//   k_cox_offsets x3, k_cox_scan x3
//                       T = suffix scan of ev by strata; (cnt, Dv) prefix-scanned and Sdv suffix-scanned by TIE GROUP: cnt[s] - 1
//                       is an event's l, cnt[last] = d, Dv[last] = D, Sdv[first] = sum dv
//   k_efron_hazard      at every event: h = m / den, h2 = h / den, hc = c h, hc2 = c^2 h2 (c = 1 - l / d), lg = log den, mm = m
//   k_cox_offsets x2, k_cox_scan x2
//                       (h, h2) prefix-scanned by strata, (hc, hc2) by tie group
//   k_efron_apply       A = hA[last] for a row that is not an event; for an event (before its group) + (its group's hc):
//                       (first > sfirst ? hA[first - 1] : 0) + hc[last]; B likewise; then cox_row's lines
// The only subtraction added is the one in den.  The work per position is constant whatever the groups' sizes.
#include "cox_efron.hpp"

#include "block_sum.hpp"

using namespace cdk;
static_assert(kCoxBlock == kBlock, "block_sum is block_sum.hpp's");
static_assert(kCoxPer == 4, "a lane holds four positions");

namespace {

// k_efron_mark: the inputs of the tie-group scans.  The runs' records are k_cox_hazard's and k_cox_exp's with the tie groups'
// bounds where the strata's stand: for the prefix scans (heads: first[s] == s) the sum over the run's positions from the first
// position of the group its last position lies in, head seen when that group starts inside the run; for the suffix scan
// (heads: last[s] == s) the sum up to the last position of the group the run starts in, head seen when it ends inside the run.
__global__ __launch_bounds__(kCoxBlock) void k_efron_mark(const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                          const double* __restrict__ eT, const double* __restrict__ hA,
                                                          int64_t ld, int64_t tiles, double* __restrict__ cnt,
                                                          double* __restrict__ Dv, double* __restrict__ Sdv,
                                                          double* __restrict__ esums, int32_t* __restrict__ heads_p,
                                                          int32_t* __restrict__ heads_s) {
    __shared__ double s_red[3 * (kCoxBlock / 64)];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int64_t end = t1 * kCoxTile < ld ? t1 * kCoxTile : ld;
    const int64_t gb = first[end - 1], ge = last[t0 * kCoxTile];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const double dv = hA[s];
            const bool event = dv != 0.0;
            const double one = event ? 1.0 : 0.0;
            const double ev = event ? eT[s] : 0.0;
            cnt[s] = one;
            Dv[s] = ev;
            Sdv[s] = dv;
            acc[0] += s >= gb ? one : 0.0;
            acc[1] += s >= gb ? ev : 0.0;
            acc[2] += s <= ge ? dv : 0.0;
        }
    }
    block_sum<3>(acc, s_red);
    if (threadIdx.x == 0) {
        esums[blockIdx.x] = acc[0];
        esums[kCoxMaxGrid + blockIdx.x] = acc[1];
        esums[2 * kCoxMaxGrid + blockIdx.x] = acc[2];
        heads_p[blockIdx.x] = gb >= t0 * kCoxTile ? 1 : 0;
        heads_s[blockIdx.x] = ge < end ? 1 : 0;
    }
}

// One event's terms, every operation rounded on its own (tests/_cox_efron_numpy.py writes the same lines).  rank = l + 1.
struct EfronTerm { double h, h2, hc, hc2, lg, m; };
__device__ __forceinline__ EfronTerm efron_term(bool event, double rank, double d, double D, double sdv, double S) {
#pragma clang fp contract(off)
    EfronTerm o;
    const double m = sdv / d;
    const double frac = (rank - 1.0) / d;
    const double den = S - frac * D;
    const bool ok = event && den > 0.0;          // an event whose den is not > 0 is skipped, as k_cox_hazard skips S
    const double cf = 1.0 - frac;
    const double h = m / den;
    const double h2 = h / den;
    o.h = ok ? h : 0.0;
    o.h2 = ok ? h2 : 0.0;
    o.hc = ok ? cf * h : 0.0;
    o.hc2 = ok ? (cf * cf) * h2 : 0.0;
    o.lg = ok ? log(den) : 0.0;
    o.m = ok ? m : 0.0;
    return o;
}

// k_efron_hazard: k_cox_hazard<true> with Efron's denominators.  hA still holds dv (k_cox_exp), eT the suffix scan T, cnt, Dv
// and Sdv their tie-group scans.  h and h2 go where k_cox_hazard puts them, with its runs' records (heads: the strata's first
// positions); hc and hc2 get the tie groups' records, whose head flags k_efron_mark has written.
__global__ __launch_bounds__(kCoxBlock) void k_efron_hazard(const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                            const int32_t* __restrict__ sfirst, const double* __restrict__ eT,
                                                            const double* __restrict__ cnt, const double* __restrict__ Dv,
                                                            const double* __restrict__ Sdv, double* __restrict__ hA,
                                                            double* __restrict__ hB, double* __restrict__ hc,
                                                            double* __restrict__ hc2, double* __restrict__ lg,
                                                            double* __restrict__ mm, int64_t ld, int64_t tiles,
                                                            double* __restrict__ sums_h, int32_t* __restrict__ heads_h,
                                                            double* __restrict__ esums) {
#pragma clang fp contract(off)
    __shared__ double s_red[4 * (kCoxBlock / 64)];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int64_t end = t1 * kCoxTile < ld ? t1 * kCoxTile : ld;
    const int64_t sb = sfirst[end - 1], gb = first[end - 1];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const int32_t f = first[s], l = last[s];
            const EfronTerm o = efron_term(hA[s] != 0.0, cnt[s], cnt[l], Dv[l], Sdv[f], eT[f]);
            hA[s] = o.h;
            hB[s] = o.h2;
            hc[s] = o.hc;
            hc2[s] = o.hc2;
            lg[s] = o.lg;
            mm[s] = o.m;
            acc[0] += s >= sb ? o.h : 0.0;
            acc[1] += s >= sb ? o.h2 : 0.0;
            acc[2] += s >= gb ? o.hc : 0.0;
            acc[3] += s >= gb ? o.hc2 : 0.0;
        }
    }
    block_sum<4>(acc, s_red);
    if (threadIdx.x == 0) {
        sums_h[blockIdx.x] = acc[0];
        sums_h[kCoxMaxGrid + blockIdx.x] = acc[1];
        esums[3 * kCoxMaxGrid + blockIdx.x] = acc[2];
        esums[4 * kCoxMaxGrid + blockIdx.x] = acc[3];
        heads_h[blockIdx.x] = sb >= t0 * kCoxTile ? 1 : 0;
    }
}

// k_efron_apply: k_cox_apply<APPLY, true> with Efron's A and B and the nll's term m log den - dv ec.  The lines from eta to z are
// cox_eta's and cox_row's (cox_kernels.hpp), with ev = v e for e and dv = v delta for delta.
template <bool APPLY>
__global__ __launch_bounds__(kCoxBlock) void k_efron_apply(const int32_t* __restrict__ order, const int32_t* __restrict__ first,
                                                           const int32_t* __restrict__ last, const int32_t* __restrict__ sfirst,
                                                           const double* __restrict__ status, double* __restrict__ y,
                                                           double* __restrict__ r, double* __restrict__ w,
                                                           const double* __restrict__ offset, const uint8_t* __restrict__ fold,
                                                           int k, int64_t n, int64_t ld, int64_t tiles, double wmin,
                                                           double eta_max, const double* __restrict__ hA,
                                                           const double* __restrict__ hB, const double* __restrict__ hc,
                                                           const double* __restrict__ hc2, const double* __restrict__ lg,
                                                           const double* __restrict__ mm, double* __restrict__ partials,
                                                           const double* __restrict__ weight) {
#pragma clang fp contract(off)
    __shared__ double s_red[kCoxVals * (kCoxBlock / 64)];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    double acc[kCoxVals] = {};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const int32_t row = order[s];
            const bool live = s < n;
            const bool held = live && fold != nullptr && (int)fold[row] == k;
            const bool train = live && !held;
            const double eta_lin = y[row] - r[row];
            const double eta = eta_lin + (offset ? offset[row] : 0.0);
            const bool capped = eta > eta_max;
            const double ec = capped ? eta_max : eta;
            const double v = weight[row];
            const double ev = v * exp(ec);
            const double dv = v * (train ? status[row] : 0.0);
            const int32_t f = first[s], l = last[s];
            double A = hA[l], B = hB[l];
            if (dv != 0.0) {                       // an event: the groups before its own, then its own group's terms with c
                const bool any = f > sfirst[s];
                A = (any ? hA[f - 1] : 0.0) + hc[l];
                B = (any ? hB[f - 1] : 0.0) + hc2[l];
            }
            const double eA = ev * A;
            const double eB = ev * B;
            const double w_raw = eA - ev * eB;
            const bool clamped = !(w_raw >= wmin);
            const double wi = clamped ? wmin : w_raw;
            const double d = dv - eA;
            const double ri = d / wi;
            const double zi = eta_lin + ri;
            const double m = mm[s];
            const double nll = m != 0.0 ? m * lg[s] - dv * ec : 0.0;
            if constexpr (APPLY) {
                w[row] = train ? wi : 0.0;
                y[row] = train ? zi : (held ? eta_lin : 0.0);
                r[row] = train ? ri : 0.0;
            }
            acc[0] += train ? nll : 0.0;
            acc[1] += train ? wi : 0.0;
            acc[2] += (train && clamped) ? 1.0 : 0.0;
            acc[3] += (live && capped) ? 1.0 : 0.0;
            acc[4] += dv;
        }
    }
    block_sum<kCoxVals>(acc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kCoxVals; ++i) partials[(int64_t)blockIdx.x * kCoxVals + i] = acc[i];
    }
}

}  // namespace

hipError_t cox_efron_mark(hipStream_t stream, const CoxPlan& pl, int64_t ld, const CoxEfronBufs& b) {
    hipLaunchKernelGGL(k_efron_mark, dim3((unsigned)pl.grid), dim3(kCoxBlock), 0, stream, b.first, b.last, (const double*)b.eT,
                       (const double*)b.hA, ld, pl.tiles, b.cnt, b.cnt + ld, b.Sdv, b.esums, b.heads_p, b.heads_s);
    return hipGetLastError();
}

hipError_t cox_efron_hazard(hipStream_t stream, const CoxPlan& pl, int64_t ld, const CoxEfronBufs& b) {
    hipLaunchKernelGGL(k_efron_hazard, dim3((unsigned)pl.grid), dim3(kCoxBlock), 0, stream, b.first, b.last, b.sfirst,
                       (const double*)b.eT, (const double*)b.cnt, (const double*)(b.cnt + ld), (const double*)b.Sdv, b.hA, b.hB,
                       b.hc, b.hc + ld, b.lg, b.mm, ld, pl.tiles, b.sums_h, b.heads_h, b.esums);
    return hipGetLastError();
}

hipError_t cox_efron_apply(hipStream_t stream, const CoxPlan& pl, const CoxEfronBufs& b, const CoxEfronRows& rw, bool apply) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid), dim3(kCoxBlock), 0, stream, b.order, b.first, b.last, b.sfirst,
                           rw.status, rw.y, rw.r, rw.w, rw.offset, rw.fold, rw.k, rw.n, rw.ld, pl.tiles, rw.wmin, rw.eta_max,
                           (const double*)b.hA, (const double*)b.hB, (const double*)b.hc, (const double*)(b.hc + rw.ld),
                           (const double*)b.lg, (const double*)b.mm, rw.partials, rw.weight);
    };
    if (apply) go(k_efron_apply<true>); else go(k_efron_apply<false>);
    return hipGetLastError();
}
