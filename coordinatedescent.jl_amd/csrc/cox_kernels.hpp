// cox_kernels.hpp -- the IRLS step of the l1-penalised Cox model with Breslow ties (no reference counterpart; a round's solve is
// the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194).  The first family whose step is not
// elementwise: with e_i = exp(eta_i), S_i = sum of e over the rows at risk at t_i, A_i = sum of delta / S and B_i = sum of
// delta / S^2 over the rows with t <= t_i, the working weight is w_i = e_i A_i - e_i^2 B_i and the gradient of the negative log
// partial likelihood in eta is -(delta_i - e_i A_i) (Simon, Friedman, Hastie, Tibshirani 2011, eq. 9-10).  Included by cdhip.hip
// inside its anonymous namespace, after glm_kernels.hpp, whose host body (glm_step), refusals and catch-up it shares; the
// tiles, the runs of the workgroups and the scratch layout are cox_plan.hpp's.
//
// The design and the handle's vectors stay in the caller's row order.  cdh_glm_set_survival sorts the times on the host and
// uploads `order` (sorted position -> row) with the bounds of every position's tie group (first, last: two int32 vectors); the
// kernels gather through order, scan in sorted space and scatter w, z and r back.  The step is a chain of plain launches on
// the handle's stream -- no workgroup waits for another, no atomics:
//   k_cox_exp       e = exp(min(eta, eta_max)) and the training status in sorted order, the sum of e per run
//   k_cox_offsets   the runs' sums into exclusive suffix offsets (one workgroup)
//   k_cox_scan      T = suffix scan of e in place;  S of a position is T at its group's first position
//   k_cox_hazard    h = delta / S, h2 = h / S in place of the status, their sums per run
//   k_cox_offsets   the runs' sums into exclusive prefix offsets (one workgroup per scan)
//   k_cox_scan      A, B = prefix scans of h, h2 in place, read at a group's last position
//   k_cox_apply     w, z, r scattered to the rows, the record's partials;  k_gram_reduce adds them in block order
// Every sum runs in a fixed order (cox_block_excl: __shfl_up over the 64 lanes, the four waves in order, the tiles of a run in
// order, the runs in order), so the step is bit-identical run to run.
//
// Strata and observation weights (cdh_glm_set_survival_strata; glmnet's stratifySurv and weights =): a row has a weight v > 0
// and a stratum id; ev = v e and dv = v delta take the places of e and delta, and S, A and B run over the rows of the row's own
// stratum.  The order is then by (stratum, time), a stratum is a SEGMENT of sorted positions (sfirst, slast: its bounds, two more
// int32 vectors), and the three scans are segmented: they restart at every head -- a stratum's last position for the suffix
// scan, its first for the prefix scans -- by the operator (f1, v1) + (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2) carried through a
// lane's four positions, cox_block_excl, the carry from tile to tile and the runs' offsets.  No sum ever crosses a boundary,
// so the rounding error of a stratum's S, A and B is relative to ITS sums, whatever the other strata hold (a plain scan with a
// subtraction at the boundary would carry n U of the later strata's sums into it).  Every kernel of the chain has the two
// instantiations, chosen on the host (glm_launch<GlmCox>): a handle without strata and weights runs today's arithmetic, and
// the additions a segmented scan does are the plain scan's in its order -- one stratum and unit weights give the same bits.
//
// Start-stop times (cdh_glm_set_survival_interval; glmnet's Surv(start, stop, status)): row i is at risk at t iff
// start_i < t <= stop_i, inside its stratum.  The order above is by (stratum, stop); a SECOND order by (stratum, start) holds
// every stratum in the same positions, ev is gathered into it (k_cox_gather: the same bits in both orders) and suffix-scanned
// there, segmented, into T2.  Two static int32 lookups made on the host (cox_order_interval) finish the sums:
//   S = T[first[s]] - T2[lo[s]]           the rows whose stop is >= the time less those whose start is too (lo = -1: none)
//   A = hA[last[s]] - hA[enter[s]]        the hazard over the event times in (start, stop]; B likewise (enter = -1: from the start)
// No scatter-add and no atomic: every sum keeps its fixed order.  The subtractions are inherent -- glmnet and survival::coxph
// subtract too -- and they stay inside the row's stratum: the error of S is relative to T + T2, about n U (T + T2), not to S,
// and that of A and B to P(stop) + P(start).  An event whose computed S is not > 0 is skipped (k_cox_hazard's convention), a
// w_raw driven negative is clamped (cox_row's !(w_raw >= wmin)).  An interval handle always runs the segmented, weighted
// arithmetic (absent strata and weights are stored as their defaults): one chain more, chosen on the host, and the plain and
// the strata instantiations are untouched.  With every lookup -1 the chain gives the strata chain's bits.
//   k_cox_exp<true>  k_cox_gather  k_cox_offsets x2  k_cox_scan (T)  k_cox_scan (T2)  k_cox_hazard_iv  k_cox_offsets
//   k_cox_scan (A, B)  k_cox_apply_iv  k_gram_reduce
// The three kernels of its own and its launcher live in cox_interval.hpp, which cdhip.hip includes LAST (the reason is there).
//
// Efron ties (cdh_glm_set_cox_ties; survival::coxph's default, right-censored data only): a fourth chain, always segmented and
// weighted like the interval chain, in which the sums over a tie group -- an event's rank, the group's events, their ev and dv
// -- are scans that restart at the tie groups' bounds: k_cox_scan<., ., true> with `first` or `last` as its heads.  Its three
// kernels are compiled in a translation unit of their own, cox_efron.hip (the mathematics and the chain are described there),
// so that this unit's code object stays what it was; its launcher, cox_efron_host.hpp, is included after cox_interval.hpp.

// One position's share of the step, every quantity in double and every operation rounded on its own (tests/_cox_numpy.py
// writes the same lines).  eta_lin = yw - r is X beta: the offset is NOT part of the stored working response.
struct CoxEta { double eta_lin, ec, e; bool capped; };
__device__ __forceinline__ CoxEta cox_eta(double yw, double r, double off, double eta_max) {
#pragma clang fp contract(off)
    CoxEta o;
    o.eta_lin = yw - r;
    const double eta = o.eta_lin + off;
    o.capped = eta > eta_max;
    o.ec = o.capped ? eta_max : eta;
    o.e = exp(o.ec);
    return o;
}

// A training row from its e, the scans read at its tie group's bounds and its status: eA = e A, w_raw = eA - e (e B) -- the
// diagonal of the Hessian, which cancels to nothing where a row is most of its risk set -- clamped below at wmin;
// d = delta - eA, r_new = d / w, z = eta_lin + r_new;  nll = delta (log S - eta), 0 where S = 0 (k_cox_hazard).  A row before the first event has A = B = 0:
// w_raw = 0 is clamped and r_new = 0 exactly.
struct CoxRow { double w, z, r, nll; bool clamped; };
__device__ __forceinline__ CoxRow cox_row(const CoxEta& t, double S, double A, double B, double delta, double wmin) {
#pragma clang fp contract(off)
    CoxRow o;
    const double eA = t.e * A;
    const double eB = t.e * B;
    const double w_raw = eA - t.e * eB;
    o.clamped = !(w_raw >= wmin);
    o.w = o.clamped ? wmin : w_raw;
    const double d = delta - eA;
    o.r = d / o.w;
    o.z = t.eta_lin + o.r;
    o.nll = (delta != 0.0 && S > 0.0) ? log(S) - t.ec : 0.0;
    return o;
}

// The exclusive scan of one value per lane over the workgroup, in lane order, and the workgroup's total: Kogge-Stone over the
// 64 lanes of a wave, the waves' totals added in wave order.  Two barriers: the first keeps the previous trip's readers of s_w
// ahead of this trip's writers.
// SEG: the segmented scan of (value, head seen) pairs under (f1, v1) + (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2) -- a lane's
// value is its sum since the last head it holds, f whether it holds one; the result is the sum since the last head among the
// lanes before this one, f becomes whether there is one, tf whether the workgroup holds any.  The additions that do happen
// are the plain scan's, in its order: without a head the bits are the same.  s_f: a flag word per wave.
template <bool SEG>
__device__ __forceinline__ double cox_block_excl(double v, double* s_w /* [kCoxBlock / 64] */, double& total, int& f,
                                                 int* s_f /* [kCoxBlock / 64] */, int& tf) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double x = v;
    int fl = f;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_up(x, d, 64);
        if constexpr (SEG) {
            const int g = __shfl_up(fl, d, 64);
            if (lane >= d) {
                if (!fl) x = t + x;
                fl |= g;
            }
        } else {
            if (lane >= d) x = t + x;
        }
    }
    double ex = __shfl_up(x, 1, 64);
    if (lane == 0) ex = 0.0;
    int exf = 0;
    if constexpr (SEG) {
        exf = __shfl_up(fl, 1, 64);
        if (lane == 0) exf = 0;
    }
    __syncthreads();
    if (lane == 63) {
        s_w[wv] = x;
        if constexpr (SEG) s_f[wv] = fl;
    }
    __syncthreads();
    double base = 0.0, all = 0.0;
    int bf = 0, af = 0;
#pragma unroll
    for (int i = 0; i < kCoxBlock / 64; ++i) {
        if constexpr (SEG) {
            const int g = s_f[i];
            if (i < wv) { base = g ? s_w[i] : base + s_w[i]; bf |= g; }
            all = g ? s_w[i] : all + s_w[i];
            af |= g;
        } else {
            if (i < wv) base += s_w[i];
            all += s_w[i];
        }
    }
    total = all;
    if constexpr (SEG) {
        tf = af;
        f = exf | bf;
        return exf ? ex : base + ex;
    }
    return base + ex;
}

// is the row at sorted position s (row `row`) live, and held out of fold k?
__device__ __forceinline__ bool cox_held(const uint8_t* __restrict__ fold, int k, int32_t row) {
    return fold != nullptr && (int)fold[row] == k;
}

// e and the training status (delta of a live row that is not held out, else 0) in sorted order; sums[b]: the sum of e over
// workgroup b's run.  A held-out row and a pad row contribute e = 0: they leave every risk set.  fold == nullptr: nobody is held.
// SW (strata and weights, cdh_glm_set_survival_strata): ev = v e and dv = v delta are stored, each product rounded on its own;
// the run's record is (the sum since the last head in scan direction, head seen): the suffix scan's heads are the strata's
// LAST positions, so the record's sum runs over the run's positions up to the end of the stratum its first position lies
// in, and a head is seen when that stratum ends inside the run.
template <bool SW>
__global__ __launch_bounds__(kCoxBlock) void k_cox_exp(const int32_t* __restrict__ order, const double* __restrict__ status,
                                                       const double* __restrict__ y, const double* __restrict__ r,
                                                       const double* __restrict__ offset, const uint8_t* __restrict__ fold, int k,
                                                       int64_t n, int64_t ld, int64_t tiles, double eta_max,
                                                       double* __restrict__ eT, double* __restrict__ hA, double* __restrict__ sums,
                                                       const double* __restrict__ weight, const int32_t* __restrict__ slast,
                                                       int32_t* __restrict__ heads) {
#pragma clang fp contract(off)
    __shared__ double s_red[kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    int64_t bound = ld;                       // SW: the last position of the stratum the run starts in
    if constexpr (SW) bound = slast[t0 * kCoxTile];
    double acc[1] = {0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const int32_t row = order[s];
            const bool train = s < n && !cox_held(fold, k, row);
            const CoxEta o = cox_eta(y[row], r[row], offset ? offset[row] : 0.0, eta_max);
            if constexpr (SW) {
                const double v = weight[row];
                const double e = train ? v * o.e : 0.0;
                eT[s] = e;
                hA[s] = train ? v * status[row] : 0.0;
                acc[0] += s <= bound ? e : 0.0;
            } else {
                const double e = train ? o.e : 0.0;
                eT[s] = e;
                hA[s] = train ? status[row] : 0.0;
                acc[0] += e;
            }
        }
    }
    block_sum<1>(acc, s_red);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = acc[0];
        if constexpr (SW) {
            const int64_t end = t1 * kCoxTile < ld ? t1 * kCoxTile : ld;
            heads[blockIdx.x] = bound < end ? 1 : 0;
        }
    }
}

// The sums of `runs` runs into exclusive offsets, in place, one workgroup per scan (blockIdx.x picks the scan, kCoxMaxGrid doubles
// apart): SUFFIX -- the sum of the later runs -- or prefix -- of the earlier ones.  A lane holds kCoxPer runs.
// SEG: the runs' records are (sum since the last head in scan direction, head seen: heads[i], one flag array for every scan of
// the launch), and the offset of a run is the sum since the last head among the runs before it in scan direction.
template <bool SUFFIX, bool SEG>
__global__ __launch_bounds__(kCoxBlock) void k_cox_offsets(double* __restrict__ sums, int runs, const int32_t* __restrict__ heads) {
    __shared__ double s_w[kCoxBlock / 64];
    __shared__ int s_f[kCoxBlock / 64];
    double* v = sums + (int64_t)blockIdx.x * kCoxMaxGrid;
    const int q = SUFFIX ? kCoxBlock - 1 - (int)threadIdx.x : (int)threadIdx.x;     // the chunk this lane holds, in scan order
    double x[kCoxPer], l[kCoxPer];
    int hd[kCoxPer], fl[kCoxPer] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int i = q * kCoxPer + c;
        x[c] = i < runs ? v[i] : 0.0;
        hd[c] = 0;
        if constexpr (SEG) hd[c] = i < runs ? heads[i] : 0;
    }
    // l[c]: the sum of the lane's values that come before c in scan order (SEG: since the last head among them, fl[c])
    double mine;
    int mf = 0;
    if constexpr (SEG) {
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
    } else {
        if (SUFFIX) { l[3] = 0.0; l[2] = x[3]; l[1] = l[2] + x[2]; l[0] = l[1] + x[1]; }
        else        { l[0] = 0.0; l[1] = x[0]; l[2] = l[1] + x[1]; l[3] = l[2] + x[2]; }
        mine = SUFFIX ? l[0] + x[0] : l[3] + x[3];
    }
    double total;
    int tf;
    const double base = cox_block_excl<SEG>(mine, s_w, total, mf, s_f, tf);
#pragma unroll
    for (int c = 0; c < kCoxPer; ++c) {
        const int i = q * kCoxPer + c;
        if (i < runs) v[i] = (SEG && fl[c]) ? l[c] : base + l[c];
    }
}
static_assert(kCoxPer == 4, "k_cox_offsets and k_cox_scan write a lane's four partial sums out");

// NV scans in place (buffers ld doubles apart from v, offsets kCoxMaxGrid apart from offs): inclusive SUFFIX scans -- v[s]
// becomes the sum over the positions >= s -- or inclusive prefix scans.  Workgroup b walks its run backwards or forwards and
// carries the sum of what it has passed, starting from its run's offset.
// SEG: the scans restart at every head -- bound[s] == s, bound the strata's last positions for the suffix scan and their first
// for the prefix scans -- through the lane's four positions, the workgroup's scan and the carry from tile to tile.
template <int NV, bool SUFFIX, bool SEG>
__global__ __launch_bounds__(kCoxBlock) void k_cox_scan(double* __restrict__ v, const double* __restrict__ offs, int64_t ld,
                                                        int64_t tiles, const int32_t* __restrict__ bound) {
    __shared__ double s_w[NV][kCoxBlock / 64];
    __shared__ int s_f[NV][kCoxBlock / 64];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    const int q = SUFFIX ? kCoxBlock - 1 - (int)threadIdx.x : (int)threadIdx.x;
    double carry[NV];
#pragma unroll
    for (int a = 0; a < NV; ++a) carry[a] = offs[(int64_t)a * kCoxMaxGrid + blockIdx.x];
    for (int64_t i = 0; i < t1 - t0; ++i) {
        const int64_t t = SUFFIX ? t1 - 1 - i : t0 + i;
        const int64_t s0 = t * kCoxTile + (int64_t)q * kCoxPer;
        const bool in = s0 < ld;
        int hd[kCoxPer] = {0, 0, 0, 0};
        if constexpr (SEG) {
            if (in) {
#pragma unroll
                for (int c = 0; c < kCoxPer; ++c) hd[c] = (int64_t)bound[s0 + c] == s0 + c;
            }
        }
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            double* va = v + (int64_t)a * ld;
            double x[kCoxPer], l[kCoxPer];
            int fl[kCoxPer] = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < kCoxPer; ++c) x[c] = in ? va[s0 + c] : 0.0;
            // l[c]: the inclusive scan inside the lane (SEG: since the last head at or before c in scan order, fl[c])
            if constexpr (SEG) {
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
            } else {
                if (SUFFIX) { l[3] = x[3]; l[2] = l[3] + x[2]; l[1] = l[2] + x[1]; l[0] = l[1] + x[0]; }
                else        { l[0] = x[0]; l[1] = l[0] + x[1]; l[2] = l[1] + x[2]; l[3] = l[2] + x[3]; }
            }
            double total;
            int f = SUFFIX ? fl[0] : fl[3], tf = 0;
            const double ex = cox_block_excl<SEG>(SUFFIX ? l[0] : l[3], s_w[a], total, f, s_f[a], tf);
            const double base = (SEG && f) ? ex : carry[a] + ex;
            if (in) {
#pragma unroll
                for (int c = 0; c < kCoxPer; ++c) va[s0 + c] = (SEG && fl[c]) ? l[c] : base + l[c];
            }
            carry[a] = (SEG && tf) ? total : carry[a] + total;
        }
    }
}

// h = delta / S and h2 = h / S over the status k_cox_exp left in hA, S = T at the group's first position; sums[b] and
// sums[kCoxMaxGrid + b]: their sums over workgroup b's run.  A position without a training event has h = h2 = 0 whatever S
// is (S = 0 behind the last training row).  eta is capped from above only: where exp underflows to 0 on every row of an
// event's risk set (eta below -745) S is 0, and that event adds no hazard here and no term to the nll in k_cox_apply -- its
// row gets eA = 0, the clamped weight and r = delta / wmin, all finite -- rather than an infinity.
// SEG: the prefix scans' heads are the strata's FIRST positions, so the run's records sum over its positions from the start of
// the stratum its last position lies in, and a head is seen (heads[b]) when that stratum starts inside the run.
template <bool SEG>
__global__ __launch_bounds__(kCoxBlock) void k_cox_hazard(const int32_t* __restrict__ first, const double* __restrict__ eT,
                                                          double* __restrict__ hA, double* __restrict__ hB, int64_t ld, int64_t tiles,
                                                          double* __restrict__ sums, const int32_t* __restrict__ sfirst,
                                                          int32_t* __restrict__ heads) {
    __shared__ double s_red[2 * (kCoxBlock / 64)];
    const int64_t t0 = cox_run_first(tiles, gridDim.x, blockIdx.x), t1 = cox_run_first(tiles, gridDim.x, blockIdx.x + 1);
    int64_t bound = 0;                        // SEG: the first position of the stratum the run ends in
    if constexpr (SEG) bound = sfirst[(t1 * kCoxTile < ld ? t1 * kCoxTile : ld) - 1];
    double acc[2] = {0.0, 0.0};
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * kCoxTile + (int64_t)threadIdx.x * kCoxPer;
        if (s0 >= ld) continue;
#pragma unroll
        for (int c = 0; c < kCoxPer; ++c) {
            const int64_t s = s0 + c;
            const double delta = hA[s];
            const double S = eT[first[s]];
            const bool haz = delta != 0.0 && S > 0.0;
            const double h = haz ? delta / S : 0.0;
            const double h2 = haz ? h / S : 0.0;
            hA[s] = h;
            hB[s] = h2;
            if constexpr (SEG) {
                acc[0] += s >= bound ? h : 0.0;
                acc[1] += s >= bound ? h2 : 0.0;
            } else {
                acc[0] += h;
                acc[1] += h2;
            }
        }
    }
    block_sum<2>(acc, s_red);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = acc[0];
        sums[kCoxMaxGrid + blockIdx.x] = acc[1];
        if constexpr (SEG) heads[blockIdx.x] = bound >= t0 * kCoxTile ? 1 : 0;
    }
}

// The rows' share.  A training row becomes (w, z, r_new) of cox_row; a held-out row gets w = 0 exactly, z = eta_lin and r = 0,
// the convention of k_glm_step; a pad row is WRITTEN as zeros with APPLY.  Every row is written by the one lane that read it
// (order is a permutation).  The record: (sum of delta (log S - eta) over the training rows, sum w, training rows clamped at
// wmin, live rows capped at eta_max, sum of dv over the training rows: the events among them, bit for bit, without weights),
// partials[b kCoxVals + i].  With APPLY = false nothing is written but the record.
// WT (observation weights v): cox_row's lines with ev = v e for e and dv = v delta for delta, every product rounded on its
// own, and the nll term dv (log S - ec): w_raw = ev A - ev (ev B), d = dv - ev A.
template <bool APPLY, bool WT>
__global__ __launch_bounds__(kCoxBlock) void k_cox_apply(const int32_t* __restrict__ order, const int32_t* __restrict__ first,
                                                         const int32_t* __restrict__ last, const double* __restrict__ status,
                                                         double* __restrict__ y, double* __restrict__ r, double* __restrict__ w,
                                                         const double* __restrict__ offset, const uint8_t* __restrict__ fold, int k,
                                                         int64_t n, int64_t ld, int64_t tiles, double wmin, double eta_max,
                                                         const double* __restrict__ eT, const double* __restrict__ hA,
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
            double delta = train ? status[row] : 0.0;
            if constexpr (WT) {
                const double v = weight[row];
                o.e = v * o.e;
                delta = v * delta;
            }
            CoxRow q = cox_row(o, eT[first[s]], hA[last[s]], hB[last[s]], delta, wmin);
            if constexpr (WT) q.nll = delta * q.nll;
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
static_assert(kCoxBlock == kBlock, "block_sum is kernels.hpp's");

// ---- the host ------------------------------------------------------------------------------------------------------------------
// cdh_glm_set_survival: leaves the handle exactly as cdh_set_y of n zeros would (what that export voids is voided here, in its
// order), the status where the labels live, the offset where the Poisson family's lives, and the Cox group -- order, the tie
// groups' bounds, the scans' scratch and the times -- allocated together and complete before the handle changes.
// cdh_glm_set_survival_strata is the same body: with strata or weights the order is by (stratum, time) and the second pair of
// buffers (cox_layout: the strata's bounds, the ids, the runs' head flags; the weights as given, pads zero) is allocated with
// the rest, all or nothing; an absent one of the two is stored as its default (stratum 0, weight 1).  Without both the calls,
// the uploads and the handle are cdh_glm_set_survival's, and strata and weights set earlier are dropped.
// cdh_glm_set_survival_interval is the same body again: with start times host_time are the stop times, the handle always holds
// the second pair (absent strata and weights as their defaults) and the THIRD (cox_layout: the start order, the two lookups,
// the second suffix scan's scratch, the starts as given), allocated with the rest, all or nothing.  Without start times it is
// cdh_glm_set_survival_strata call for call, and every setter without them drops start times set earlier.
int32_t cox_set_survival(cdh_handle h, const void* host_time, const void* host_status, const void* host_offset,
                         const int32_t* host_strata = nullptr, const void* host_weights = nullptr,
                         const void* host_start = nullptr) {
    CHK(glm_refuse(h));
    if (!host_time) return fail(h, CDH_BAD_ARG, "host_time is NULL");
    if (!host_status) return fail(h, CDH_BAD_ARG, "host_status is NULL");
    const double* tm = (const double*)host_time;
    const double* st = (const double*)host_status;
    const double* off = (const double*)host_offset;
    const double* wt = (const double*)host_weights;
    const double* sta = (const double*)host_start;
    const bool iv = sta != nullptr;
    // the tie rule stays (cdh_glm_set_cox_ties) unless start times come: an Efron handle stores absent strata and weights as
    // their defaults, like an interval handle; its Efron pair is already there
    const bool ef = h->glm.set && h->glm.family == GlmData::Cox && h->glm.cox.efron && !iv;
    const bool sw = host_strata != nullptr || wt != nullptr || iv || ef;
    char buf[160];
    if (!cox_check(h->n, tm, st, off, buf, sizeof buf, wt)) return fail(h, CDH_BAD_ARG, buf);
    if (iv && !cox_check_interval(h->n, sta, tm, buf, sizeof buf)) return fail(h, CDH_BAD_ARG, buf);
    std::vector<int32_t> order, first, last, sfirst, slast, order2, pos2, lo, enter;
    if (iv) cox_order_interval(h->n, h->ld, sta, tm, host_strata, order, first, last, sfirst, slast, order2, pos2, lo, enter);
    else if (sw) cox_order_strata(h->n, h->ld, tm, host_strata, order, first, last, sfirst, slast);
    else cox_order(h->n, h->ld, tm, order, first, last);
    HIPCHK(h, hipSetDevice(h->device));
    const CoxLayout lay = cox_layout(h->ld);
    const size_t colbytes = (size_t)h->ld * sizeof(double), idxbytes = (size_t)h->ld * sizeof(int32_t);
    DevBuf<double> fresh, fresh_off, fresh_d, fresh_sd, fresh_vd;     // complete before the handle changes: a failed allocation leaves it as it was
    DevBuf<int32_t> fresh_i, fresh_si, fresh_vi;
    if (!h->glm.labels) {
        HIPCHK(h, fresh.alloc(colbytes));
        HIPCHK(h, hipMemsetAsync(fresh, 0, colbytes, h->stream));
    }
    if (off && !h->glm.offset) {
        HIPCHK(h, fresh_off.alloc(colbytes));
        HIPCHK(h, hipMemsetAsync(fresh_off, 0, colbytes, h->stream));
    }
    if (!h->glm.cox.d) {
        HIPCHK(h, fresh_d.alloc((size_t)lay.doubles * sizeof(double)));
        HIPCHK(h, fresh_i.alloc((size_t)lay.ints * sizeof(int32_t)));
        HIPCHK(h, hipMemsetAsync(fresh_d, 0, (size_t)lay.doubles * sizeof(double), h->stream));
    }
    if (sw && !h->glm.cox.sd) {
        HIPCHK(h, fresh_sd.alloc((size_t)lay.strata_doubles * sizeof(double)));
        HIPCHK(h, fresh_si.alloc((size_t)lay.strata_ints * sizeof(int32_t)));
        HIPCHK(h, hipMemsetAsync(fresh_sd, 0, (size_t)lay.strata_doubles * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(fresh_si, 0, (size_t)lay.strata_ints * sizeof(int32_t), h->stream));
    }
    if (iv && !h->glm.cox.vd) {
        HIPCHK(h, fresh_vd.alloc((size_t)lay.interval_doubles * sizeof(double)));
        HIPCHK(h, fresh_vi.alloc((size_t)lay.interval_ints * sizeof(int32_t)));
        HIPCHK(h, hipMemsetAsync(fresh_vd, 0, (size_t)lay.interval_doubles * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(fresh_vi, 0, (size_t)lay.interval_ints * sizeof(int32_t), h->stream));
    }
    h->rs.overwritten_with_y();          // r = copy(y) = 0 below
    gc_invalidate(h, false);
    h->gc.st.yy_void();
    h->small.c_valid = false;
    if (!h->glm.labels) h->glm.labels = std::move(fresh);
    if (off && !h->glm.offset) h->glm.offset = std::move(fresh_off);
    if (!h->glm.cox.d) { h->glm.cox.d = std::move(fresh_d); h->glm.cox.i = std::move(fresh_i); }
    if (sw && !h->glm.cox.sd) { h->glm.cox.sd = std::move(fresh_sd); h->glm.cox.si = std::move(fresh_si); }
    if (iv && !h->glm.cox.vd) { h->glm.cox.vd = std::move(fresh_vd); h->glm.cox.vi = std::move(fresh_vi); }
    h->glm.cox.cd = DevBuf<double>();    // the concordance group goes with the order it was derived from (cox_concordance_host.hpp)
    h->glm.cox.ci = DevBuf<int32_t>();
    double* d = h->glm.cox.d;
    int32_t* ii = h->glm.cox.i;
    HIPCHK(h, hipMemcpyAsync(h->glm.labels, st, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (off) HIPCHK(h, hipMemcpyAsync(h->glm.offset, off, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d + lay.time, tm, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(ii + lay.order, order.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(ii + lay.first, first.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(ii + lay.last, last.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
    std::vector<int32_t> ids;            // (alive until the synchronise below)
    std::vector<double> ones;
    if (sw) {
        double* sd = h->glm.cox.sd;
        int32_t* si = h->glm.cox.si;
        if (!host_strata) ids.assign((size_t)h->n, 0);
        if (!wt) ones.assign((size_t)h->n, 1.0);
        HIPCHK(h, hipMemcpyAsync(si + lay.sfirst, sfirst.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(si + lay.slast, slast.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(si + lay.strata, host_strata ? host_strata : ids.data(), (size_t)h->n * sizeof(int32_t),
                                 hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(sd + lay.weight, wt ? wt : ones.data(), (size_t)h->n * sizeof(double), hipMemcpyHostToDevice,
                                 h->stream));
    }
    if (iv) {
        double* vd = h->glm.cox.vd;
        int32_t* vi = h->glm.cox.vi;
        HIPCHK(h, hipMemcpyAsync(vi + lay.pos2, pos2.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(vi + lay.lo, lo.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(vi + lay.enter, enter.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(vd + lay.start, sta, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipMemsetAsync(h->y, 0, colbytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->r, 0, colbytes, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (the host vectors above are pageable: the copies are done here)
    h->y_set = true;
    h->glm.family = GlmData::Cox;
    h->glm.has_offset = off != nullptr;
    h->glm.cox.strata = sw;
    h->glm.cox.interval = iv;
    h->glm.cox.efron = ef;
    h->glm.weighted = false;             // (the weights of cdh_glm_set_weights go with the labels or counts they came with)
    h->glm.set = true;
    return CDH_OK;
}

int32_t cox_get_survival(cdh_handle h, void* host_time, void* host_status) {
    if (!host_time && !host_status) return fail(h, CDH_BAD_ARG, "host_time and host_status are both NULL");
    if (!h->glm.set || h->glm.family != GlmData::Cox)
        return fail(h, CDH_BAD_ARG, "no survival data are set: call cdh_glm_set_survival first");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)h->n * sizeof(double);
    if (host_time)
        HIPCHK(h, hipMemcpyAsync(host_time, (const double*)h->glm.cox.d + cox_layout(h->ld).time, bytes, hipMemcpyDeviceToHost, h->stream));
    if (host_status) HIPCHK(h, hipMemcpyAsync(host_status, h->glm.labels, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// cdh_glm_get_survival_start: the start times in the caller's row order; refused when the handle holds none
int32_t cox_get_survival_start(cdh_handle h, void* host_start) {
    NEED_P(h, host_start);
    if (!h->glm.set || h->glm.family != GlmData::Cox || !h->glm.cox.interval)
        return fail(h, CDH_BAD_ARG, "no start times are set: call cdh_glm_set_survival_interval with host_start first");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(host_start, (const double*)h->glm.cox.vd + cox_layout(h->ld).start, (size_t)h->n * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// cdh_glm_get_survival_strata: the stratum ids and the weights in the caller's row order; zeros and ones where the handle
// holds none
int32_t cox_get_survival_strata(cdh_handle h, int32_t* host_strata, void* host_weights) {
    if (!host_strata && !host_weights) return fail(h, CDH_BAD_ARG, "host_strata and host_weights are both NULL");
    if (!h->glm.set || h->glm.family != GlmData::Cox)
        return fail(h, CDH_BAD_ARG, "no survival data are set: call cdh_glm_set_survival first");
    if (!h->glm.cox.strata) {
        if (host_strata) memset(host_strata, 0, (size_t)h->n * sizeof(int32_t));
        if (host_weights) std::fill_n((double*)host_weights, (size_t)h->n, 1.0);
        return CDH_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const CoxLayout lay = cox_layout(h->ld);
    if (host_strata)
        HIPCHK(h, hipMemcpyAsync(host_strata, (const int32_t*)h->glm.cox.si + lay.strata, (size_t)h->n * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, h->stream));
    if (host_weights)
        HIPCHK(h, hipMemcpyAsync(host_weights, (const double*)h->glm.cox.sd + lay.weight, (size_t)h->n * sizeof(double),
                                 hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// cdh_glm_set_cox_ties: 0 Breslow, 1 Efron (cox_efron.hip).  Efron's chain is segmented and weighted, so a handle without strata
// and weights gets the second pair here, filled with the defaults cox_set_survival would store (one stratum over the rows, one
// over the pads, the ids zero, the weights one: cox_order_strata without ids IS cox_order, so order, first and last stay), and
// the Efron pair; all of it allocated before the handle changes.  Back at Breslow such a handle runs the segmented chain over
// its defaults, whose bits are the plain chain's.  The rows' y, w and r are not touched.
int32_t cox_set_ties(cdh_handle h, int32_t ties) {
    if (!h->glm.set || h->glm.family != GlmData::Cox)
        return fail(h, CDH_BAD_ARG, "no survival data are set: call cdh_glm_set_survival first");
    if (ties != 0 && ties != 1) return fail(h, CDH_BAD_ARG, "ties must be 0 (Breslow) or 1 (Efron)");
    if (ties == 1 && h->glm.cox.interval)
        return fail(h, CDH_BAD_ARG, "Efron ties are not offered with start-stop times: the handle holds start times");
    if (ties == 0 || h->glm.cox.efron) {
        h->glm.cox.efron = ties == 1;
        return CDH_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const CoxLayout lay = cox_layout(h->ld);
    const CoxEfronLayout el = cox_efron_layout(h->ld);
    const bool fill = !h->glm.cox.strata;
    DevBuf<double> fresh_sd, fresh_ed;
    DevBuf<int32_t> fresh_si, fresh_ei;
    if (fill && !h->glm.cox.sd) {
        HIPCHK(h, fresh_sd.alloc((size_t)lay.strata_doubles * sizeof(double)));
        HIPCHK(h, fresh_si.alloc((size_t)lay.strata_ints * sizeof(int32_t)));
    }
    if (!h->glm.cox.ed) {
        HIPCHK(h, fresh_ed.alloc((size_t)el.doubles * sizeof(double)));
        HIPCHK(h, fresh_ei.alloc((size_t)el.ints * sizeof(int32_t)));
        HIPCHK(h, hipMemsetAsync(fresh_ed, 0, (size_t)el.doubles * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(fresh_ei, 0, (size_t)el.ints * sizeof(int32_t), h->stream));
    }
    if (fill) {
        double* sd = fresh_sd ? (double*)fresh_sd : (double*)h->glm.cox.sd;
        int32_t* si = fresh_si ? (int32_t*)fresh_si : (int32_t*)h->glm.cox.si;
        std::vector<int32_t> sfirst, slast;
        cox_one_stratum(h->n, h->ld, sfirst, slast);
        std::vector<double> ones((size_t)h->ld, 0.0);
        std::fill_n(ones.begin(), (size_t)h->n, 1.0);
        const size_t idxbytes = (size_t)h->ld * sizeof(int32_t);
        HIPCHK(h, hipMemsetAsync(si, 0, (size_t)lay.strata_ints * sizeof(int32_t), h->stream));
        HIPCHK(h, hipMemcpyAsync(si + lay.sfirst, sfirst.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(si + lay.slast, slast.data(), idxbytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(sd + lay.weight, ones.data(), (size_t)h->ld * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));      // (the host vectors are pageable: the copies are done here)
    }
    if (fresh_sd) { h->glm.cox.sd = std::move(fresh_sd); h->glm.cox.si = std::move(fresh_si); }
    if (fresh_ed) { h->glm.cox.ed = std::move(fresh_ed); h->glm.cox.ei = std::move(fresh_ei); }
    h->glm.cox.strata = true;
    h->glm.cox.efron = true;
    return CDH_OK;
}

int32_t cox_get_ties(cdh_handle h, int32_t* ties) {
    NEED_P(h, ties);
    if (!h->glm.set || h->glm.family != GlmData::Cox)
        return fail(h, CDH_BAD_ARG, "no survival data are set: call cdh_glm_set_survival first");
    *ties = h->glm.cox.efron ? 1 : 0;
    return CDH_OK;
}

// The Cox family as glm_step sees it: what its export refuses, in cdh_glm_poisson_irls' order and words.
struct GlmCox {
    static constexpr int kVals = kCoxVals;
    static constexpr bool kFold = true, kOffset = true;
    static constexpr GlmData kData = GlmData::Cox;
    static constexpr bool kKBeforeOut = true;
    static constexpr const char* kOutNull = "out5 is NULL";
    static int32_t refuse_observations(cdh_handle h) {
        if (!h->glm.set || h->glm.family != kData)
            return fail(h, CDH_BAD_ARG, "cdh_glm_cox_irls needs survival data: call cdh_glm_set_survival first");
        return CDH_OK;
    }
    static int32_t refuse_params(cdh_handle h, const GlmParams& pm) { return GlmPoisson::refuse_params(h, pm); }
};

// glm_check with the Cox plan's records where the elementwise step's stand
template <>
int32_t glm_check<GlmCox>(cdh_handle h, int32_t k, int32_t apply, const GlmParams& pm, const double* out) {
    CHK(glm_refuse(h));
    CHK(GlmCox::refuse_observations(h));
    if (apply != 0 && apply != 1) return fail(h, CDH_BAD_ARG, "apply must be 0 or 1");
    CHK(GlmCox::refuse_params(h, pm));
    CHK(glm_refuse_k(h, k));
    if (!out) return fail(h, CDH_BAD_ARG, GlmCox::kOutNull);
    if ((size_t)(cox_plan(h->ld, h->knobs.cox_grid).records * kCoxVals) > h->sz.partials_doubles)
        return fail(h, CDH_BAD_ARG, "partials too small");
    return CDH_OK;
}

// the chain of a handle with start times, up to the partials (cox_interval.hpp, at the end of cdhip.hip)
int32_t cox_launch_interval(cdh_handle h, int32_t k, bool apply, const GlmParams& pm);
// the chain of a handle set to Efron ties, up to the partials (cox_efron_host.hpp, at the end of cdhip.hip)
int32_t cox_launch_efron(cdh_handle h, int32_t k, bool apply, const GlmParams& pm);

// the chain and its record: out holds the kCoxVals doubles, added over the workgroups in block order; k = -1: no row is held
// out and the fold ids are not read
template <>
int32_t glm_launch<GlmCox>(cdh_handle h, int32_t k, bool apply, const GlmParams& pm, double* out) {
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
    // the instantiations are chosen here: a handle without strata and weights runs the plain scans and the unweighted rows
    auto chain = [&](auto sw_tag) -> int32_t {
        constexpr bool SW = decltype(sw_tag)::value;
        const int32_t* si = SW ? (const int32_t*)h->glm.cox.si : (const int32_t*)nullptr;
        const int32_t *sfirst = SW ? si + lay.sfirst : nullptr, *slast = SW ? si + lay.slast : nullptr;
        int32_t* heads = SW ? (int32_t*)h->glm.cox.si + lay.heads : nullptr;
        int32_t* heads_h = SW ? heads + kCoxMaxGrid : nullptr;
        const double* weight = SW ? (const double*)h->glm.cox.sd + lay.weight : (const double*)nullptr;
        hipLaunchKernelGGL(k_cox_exp<SW>, grid, block, 0, h->stream, order, status, (const double*)y, (const double*)r, off, fold,
                           (int)k, h->n, h->ld, pl.tiles, pm.eta_max, eT, hA, sums, weight, slast, heads);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL((k_cox_offsets<true, SW>), one, block, 0, h->stream, sums, (int)pl.grid, (const int32_t*)heads);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL((k_cox_scan<1, true, SW>), grid, block, 0, h->stream, eT, (const double*)sums, h->ld, pl.tiles, slast);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(k_cox_hazard<SW>, grid, block, 0, h->stream, first, (const double*)eT, hA, hB, h->ld, pl.tiles, sums_h,
                           sfirst, heads_h);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL((k_cox_offsets<false, SW>), two, block, 0, h->stream, sums_h, (int)pl.grid, (const int32_t*)heads_h);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL((k_cox_scan<2, false, SW>), grid, block, 0, h->stream, hA, (const double*)sums_h, h->ld, pl.tiles, sfirst);
        HIPCHK(h, hipGetLastError());
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, order, first, last, status, y, r, w, off, fold, (int)k, h->n, h->ld,
                               pl.tiles, pm.wmin, pm.eta_max, (const double*)eT, (const double*)hA, (const double*)hB,
                               (double*)h->d_partials, weight);
        };
        if (apply) go(k_cox_apply<true, SW>); else go(k_cox_apply<false, SW>);
        HIPCHK(h, hipGetLastError());
        return CDH_OK;
    };
    if (h->glm.cox.efron) CHK(cox_launch_efron(h, k, apply, pm));            // cox_efron_host.hpp
    else if (h->glm.cox.interval) CHK(cox_launch_interval(h, k, apply, pm));      // cox_interval.hpp
    else if (h->glm.cox.strata) CHK(chain(std::true_type{})); else CHK(chain(std::false_type{}));
    hipLaunchKernelGGL(k_gram_reduce, dim3((kCoxVals + kReduceVals - 1) / kReduceVals), dim3(64 * kReduceWaves), 0, h->stream,
                       (const double*)h->d_partials, (int)pl.records, (int)kCoxVals, (double*)h->d_red);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_red, sizeof(double) * kCoxVals, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}
