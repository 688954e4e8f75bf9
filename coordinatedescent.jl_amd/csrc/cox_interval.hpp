// cox_interval.hpp -- the Cox step of a handle with start-stop times (cdh_glm_set_survival_interval): the three kernels the
// chain adds to cox_kernels.hpp's and its launcher.  The mathematics, the two lookups and the chain are described at the top of
// cox_kernels.hpp; the order, the lookups and the third pair of buffers are cox_plan.hpp's (cox_order_interval, cox_layout).
// Always segmented and weighted: absent strata and weights are stored as their defaults, so there is ONE interval chain.
//
// Why a file of its own, included LAST by cdhip.hip, and why k_cox_gather and k_cox_hazard_iv are templates (LATE has no
// meaning): the compiler lays a code object out in the order it emits the kernels -- a plain kernel where it is defined, a
// template where it is first used, all plain ones first.  Defined in cox_kernels.hpp as plain kernels, these sat in front of
// every template of the library and moved k_gramstep and all later kernels by 17 KB; with not one instruction of them changed
// the flagship benchmark then ran 2.5 % slower (LAB_NOTES "Cox lasso: start-stop times").  As templates first used here, they
// are emitted after every other kernel, and every other kernel keeps the address it had.
//
// That is not enough: the four new kernels' descriptors and argument metadata sit in FRONT of the code (.note, .dynsym, .rodata)
// and push all of it by 0x2a00 bytes, and at that offset k_gramstep measured 8 % slower (26.0 - 26.8 ms a sweep became 28.4 -
// 28.8) -- again with identical instructions.  The pad below lies in .rodata and rounds the push up to 0x10000, the size of the
// instruction cache, so that every existing kernel keeps every address bit below 64 KB.  It is read by nothing.  Its size
// belongs to this set of kernels and their signatures: whoever adds or changes one re-derives it from the section table
// (llvm-readelf -S of the code object: .text must move by a multiple of 0x10000 against the parent's).
__device__ __attribute__((used)) const unsigned char k_code_object_pad[0x10000 - 0x2a00] = {1};

// a[at] - (sub >= 0 ? b[sub] : 0): a scan read at its bound less the share of the rows that are not (yet) at risk.  ONE rounded
// subtraction, the same expression in k_cox_hazard_iv and k_cox_apply_iv, so that S is the same bits in both; with sub = -1 it
// is a[at], bit for bit.
__device__ __forceinline__ double cox_less(const double* a, int32_t at, const double* b, int32_t sub) {
#pragma clang fp contract(off)
    return a[at] - (sub >= 0 ? b[sub] : 0.0);
}

// T2[s] = ev of the row at start-order position s, copied from the stop order through pos2 BEFORE the suffix scan overwrites
// eT: the same bits in both orders.  sums2[b], heads2[b]: the run's record as k_cox_exp<true> writes it (a stratum holds the
// same positions in both orders, so slast bounds it here too).
template <int LATE = 0>
__global__ __launch_bounds__(kCoxBlock) void k_cox_gather(const int32_t* __restrict__ pos2, const double* __restrict__ eT,
                                                          const int32_t* __restrict__ slast, int64_t ld, int64_t tiles,
                                                          double* __restrict__ T2, double* __restrict__ sums2,
                                                          int32_t* __restrict__ heads2) {
    __shared__ double s_red[kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int64_t bound = slast[t0 * kCoxTile];
    double acc[1] = {0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const double e = eT[pos2[s]];
            T2[s] = e;
            acc[0] += s <= bound ? e : 0.0;
        }
    }
    block_sum<1>(acc, s_red);
    if (threadIdx.x == 0) {
        const int64_t end = t1 * kCoxTile < ld ? t1 * kCoxTile : ld;
        sums2[blockIdx.x] = acc[0];
        heads2[blockIdx.x] = bound < end ? 1 : 0;
    }
}

// k_cox_hazard<true> with S = T[first[s]] - T2[lo[s]]: the rows of the stratum whose stop is >= the time less those whose
// start is too.  The difference of two sums of up to n terms: its error is relative to T + T2, not to S, and where it comes out
// not > 0 the event is skipped like one whose risk set underflowed.
template <int LATE = 0>
__global__ __launch_bounds__(kCoxBlock) void k_cox_hazard_iv(const int32_t* __restrict__ first, const int32_t* __restrict__ lo,
                                                             const double* __restrict__ eT, const double* __restrict__ T2,
                                                             double* __restrict__ hA, double* __restrict__ hB, int64_t ld,
                                                             int64_t tiles, double* __restrict__ sums,
                                                             const int32_t* __restrict__ sfirst, int32_t* __restrict__ heads) {
#pragma clang fp contract(off)
    __shared__ double s_red[2 * (kCoxBlock / 64)];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int64_t bound = sfirst[(t1 * kCoxTile < ld ? t1 * kCoxTile : ld) - 1];
    double acc[2] = {0.0, 0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const double delta = hA[s];
            const double S = cox_less(eT, first[s], T2, lo[s]);
            const bool haz = delta != 0.0 && S > 0.0;
            const double h = haz ? delta / S : 0.0;
            const double h2 = haz ? h / S : 0.0;
            hA[s] = h;
            hB[s] = h2;
            acc[0] += s >= bound ? h : 0.0;
            acc[1] += s >= bound ? h2 : 0.0;
        }
    }
    block_sum<2>(acc, s_red);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = acc[0];
        sums[kCoxMaxGrid + blockIdx.x] = acc[1];
        heads[blockIdx.x] = bound >= t0 * kCoxTile ? 1 : 0;
    }
}

// k_cox_apply<APPLY, true> with S as above and A = hA[last[s]] - hA[enter[s]], B likewise: the hazard summed over the event times
// in (start, stop].  Differences again, relative to P(stop) + P(start); a w_raw driven negative is clamped by cox_row.
template <bool APPLY>
__global__ __launch_bounds__(kCoxBlock) void k_cox_apply_iv(const int32_t* __restrict__ order, const int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ last, const int32_t* __restrict__ lo,
                                                            const int32_t* __restrict__ enter, const double* __restrict__ status,
                                                            double* __restrict__ y, double* __restrict__ r, double* __restrict__ w,
                                                            const double* __restrict__ offset, const uint8_t* __restrict__ fold,
                                                            int k, int64_t n, int64_t ld, int64_t tiles, double wmin,
                                                            double eta_max, const double* __restrict__ eT,
                                                            const double* __restrict__ T2, const double* __restrict__ hA,
                                                            const double* __restrict__ hB, double* __restrict__ partials,
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
            const bool held = live && cox_held(fold, k, row);
            const bool train = live && !held;
            CoxEta o = cox_eta(y[row], r[row], offset ? offset[row] : 0.0, eta_max);
            const double v = weight[row];
            o.e = v * o.e;
            const double delta = v * (train ? status[row] : 0.0);
            const int32_t l = last[s], en = enter[s];
            CoxRow q = cox_row(o, cox_less(eT, first[s], T2, lo[s]), cox_less(hA, l, hA, en), cox_less(hB, l, hB, en), delta, wmin);
            q.nll = delta * q.nll;
            if constexpr (APPLY) {
                w[row] = train ? q.w : 0.0;
                y[row] = train ? q.z : (held ? o.eta_lin : 0.0);
                r[row] = train ? q.r : 0.0;
            }
            acc[0] += train ? q.nll : 0.0;
            acc[1] += train ? q.w : 0.0;
            acc[2] += (train && q.clamped) ? 1.0 : 0.0;
            acc[3] += (live && o.capped) ? 1.0 : 0.0;
            acc[4] += delta;
        }
    }
    block_sum<kCoxVals>(acc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kCoxVals; ++i) partials[(int64_t)blockIdx.x * kCoxVals + i] = acc[i];
    }
}

// ---- the host ------------------------------------------------------------------------------------------------------------------
// The chain up to the partials of k_cox_apply_iv; glm_launch<GlmCox> (cox_kernels.hpp) reduces and reads them back.
int32_t cox_launch_interval(cdh_handle h, int32_t k, bool apply, const GlmParams& pm) {
    const CoxPlan pl = cox_plan(h->ld, h->knobs.cox_grid);
    const CoxLayout lay = cox_layout(h->ld);
    double* d = h->glm.cox.d;
    const int32_t* ii = h->glm.cox.i;
    const int32_t *order = ii + lay.order, *first = ii + lay.first, *last = ii + lay.last;
    double *eT = d + lay.eT, *hA = d + lay.hA, *hB = d + lay.hB, *sums = d + lay.sums, *sums_h = d + lay.sums + kCoxMaxGrid;
    const double* status = h->glm.labels;
    const double* off = h->glm.has_offset ? (const double*)h->glm.offset : (const double*)nullptr;
    const uint8_t* fold = k >= 0 ? (const uint8_t*)h->cv.fold : (const uint8_t*)nullptr;
    double *y = (double*)h->y, *r = (double*)h->r, *w = (double*)h->w;
    const dim3 grid((unsigned)pl.grid), one(1), two(2), block(kCoxBlock);
    const int32_t *si = h->glm.cox.si, *vi = h->glm.cox.vi;
    const int32_t *sfirst = si + lay.sfirst, *slast = si + lay.slast;
    const int32_t *pos2 = vi + lay.pos2, *lo = vi + lay.lo, *enter = vi + lay.enter;
    int32_t *heads = (int32_t*)h->glm.cox.si + lay.heads, *heads_h = heads + kCoxMaxGrid;
    int32_t* heads2 = (int32_t*)h->glm.cox.vi + lay.heads2;
    double *T2 = (double*)h->glm.cox.vd + lay.T2, *sums2 = (double*)h->glm.cox.vd + lay.sums2;
    const double* weight = (const double*)h->glm.cox.sd + lay.weight;
    hipLaunchKernelGGL(k_cox_exp<true>, grid, block, 0, h->stream, order, status, (const double*)y, (const double*)r, off, fold,
                       (int)k, h->n, h->ld, pl.tiles, pm.eta_max, eT, hA, sums, weight, slast, heads);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_cox_gather<>, grid, block, 0, h->stream, pos2, (const double*)eT, slast, h->ld, pl.tiles, T2, sums2, heads2);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_offsets<true, true>), one, block, 0, h->stream, sums, (int)pl.grid, (const int32_t*)heads);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_offsets<true, true>), one, block, 0, h->stream, sums2, (int)pl.grid, (const int32_t*)heads2);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_scan<1, true, true>), grid, block, 0, h->stream, eT, (const double*)sums, h->ld, pl.tiles, slast);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_scan<1, true, true>), grid, block, 0, h->stream, T2, (const double*)sums2, h->ld, pl.tiles, slast);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_cox_hazard_iv<>, grid, block, 0, h->stream, first, lo, (const double*)eT, (const double*)T2, hA, hB, h->ld,
                       pl.tiles, sums_h, sfirst, heads_h);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_offsets<false, true>), two, block, 0, h->stream, sums_h, (int)pl.grid, (const int32_t*)heads_h);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_scan<2, false, true>), grid, block, 0, h->stream, hA, (const double*)sums_h, h->ld, pl.tiles, sfirst);
    HIPCHK(h, hipGetLastError());
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, order, first, last, lo, enter, status, y, r, w, off, fold, (int)k,
                           h->n, h->ld, pl.tiles, pm.wmin, pm.eta_max, (const double*)eT, (const double*)T2, (const double*)hA,
                           (const double*)hB, (double*)h->d_partials, weight);
    };
    if (apply) go(k_cox_apply_iv<true>); else go(k_cox_apply_iv<false>);
    HIPCHK(h, hipGetLastError());
    return CDH_OK;
}
