// glm_kernels.hpp -- the step between two rounds of IRLS for an l1-penalised GLM (no reference counterpart; a round's solve
// is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194): from the linear predictor the handle's
// residual stands for, the working weights, the working response and the new residual in one pass over the rows, with the
// sums a caller needs of it.  Included by cdhip.hip inside its anonymous namespace, after the handle; the grid and the rows of
// a workgroup are glm_plan.hpp's.  One kernel (k_glm_step) and one host body (glm_step) serve every family; a family -- the
// binomial, the binomial inside a fold, the Poisson with an offset, and the last two with observation weights -- is a struct
// that names its row function, its record and what its export refuses.

// One row, every quantity in double and every operation rounded on its own (no contraction into FMAs: tests/_logistic_numpy.py
// writes the same lines).  eta = yw - r;  a = |eta|, e = exp(-a);  p = 1 / (1 + e) or e / (1 + e) by the sign of eta and
// q = 1 - p from the OTHER branch, never as a difference;  w = max(e / (1 + e)^2, wmin);  d = y q - (1 - y) p, which is
// y - p without cancellation;  r_new = d / w, z = eta + r_new;  nll = max(eta, 0) + log1p(e) - y eta, log1p(e) being e itself
// where 1 + e == 1.
struct GlmRow { double w, z, r, nll; bool clamped; };
__device__ __forceinline__ GlmRow glm_row(double label, double yw, double r, double wmin) {
#pragma clang fp contract(off)
    const double eta = yw - r;
    const double a = fabs(eta), e = exp(-a);
    const double ope = 1.0 + e;
    const double big = 1.0 / ope, small = e / ope;
    const double p = eta >= 0.0 ? big : small, q = eta >= 0.0 ? small : big;
    const double w_raw = e / (ope * ope);
    GlmRow o;
    o.clamped = w_raw < wmin;
    o.w = o.clamped ? wmin : w_raw;
    const double d = label * q - (1.0 - label) * p;
    o.r = d / o.w;
    o.z = eta + o.r;
    // Where 1 + e rounds to 1 (e <= 2^-53) log1p(e) = e - e^2 / 2 + ... rounds to e, and e is taken as it is: the library's
    // log1p has no such shortcut and halves its argument on the way, which costs a subnormal e its last bit where that is odd
    // (measured: nll of a label-0 row 2^-1074 off e at eta = -708.4 and -740, and 0 instead of 2^-1074 from -744.44 to -745.13).
    // log1p is evaluated on every row and the result selected: written as `ope == 1.0 ? e : log1p(e)` the compiler branches round
    // the call, and the kernels go from 61 / 70 to 88 / 92 VGPRs and from 8 / 7 to 5 waves per SIMD (1.05x the time at n = 1e7).
    const double l1p_lib = log1p(e);
    const double l1p = __builtin_expect(ope == 1.0, 0) ? e : l1p_lib;
    o.nll = (fmax(eta, 0.0) + l1p) - label * eta;
    return o;
}

// ---- the Poisson family: counts y_i >= 0 with mean exp(x_i'beta + o_i), o the offset (log exposure) ----------------------------
// One row, every quantity in double and every operation rounded on its own (tests/_poisson_numpy.py writes the same lines).
// eta_lin = yw - r is X beta: the offset is NOT part of the stored working response, so that y_w - r stays the linear
// predictor of the columns for every later reader.  eta = eta_lin + o, capped above at eta_max (exp and w x^2 stay finite);
// mu = exp(min(eta, eta_max));  w = max(mu, wmin) -- only the weight is clamped, so X'W r = X'(y - mu) whatever W is;
// d = y - mu, r_new = d / w, z_lin = eta_lin + r_new;  nll = mu - y ec (without the log y! of the likelihood);
// dev = 2 ((y > 0 ? y log(y / mu) : 0) - (y - mu)), the row's deviance.
struct PoisRow { double w, z, r, nll, dev, eta_lin; bool clamped, capped; };
__device__ __forceinline__ PoisRow pois_row(double count, double yw, double r, double off, double wmin, double eta_max) {
#pragma clang fp contract(off)
    PoisRow o;
    o.eta_lin = yw - r;
    const double eta = o.eta_lin + off;
    o.capped = eta > eta_max;
    const double ec = o.capped ? eta_max : eta;
    const double mu = exp(ec);
    o.clamped = mu < wmin;
    o.w = o.clamped ? wmin : mu;
    const double d = count - mu;
    o.r = d / o.w;
    o.z = o.eta_lin + o.r;
    o.nll = mu - count * ec;
    const double ylog = count > 0.0 ? count * log(count / mu) : 0.0;
    o.dev = 2.0 * (ylog - d);
    return o;
}

// ---- the families ----------------------------------------------------------------------------------------------------------------
// what a step is told beside the handle: the floor of the weights and, for the Poisson family, the cap of eta
struct GlmParams { double wmin, eta_max; };

// A family names, for the kernel: kVals, the doubles of its record (glm_plan.hpp); kFold, whether a fold byte per row can hold
// rows out; kOffset, whether a fourth 16-byte stream, the offset, is read; kWeights, whether one more 16-byte stream, the
// observation weights v, is read -- o.w is then v times the family's clamped weight when add() sees it; row(), one row's
// quantities; add(), the row's terms of the record, acc[0] first -- v: the row's observation weight (1 without kWeights),
// live: the row lies below n, held: it is held out, train: live and not held.  For the host:
// kData, the observations its export needs on the handle; kKBeforeOut, whether that export looks at k before its output
// pointer; and what it refuses of the handle's observations, of the parameters and of a null output, in its own words.
//
// The binomial step: the record is (sum nll, sum w, clamped rows).  No fold byte, no offset: the step logisticLasso runs every
// round stays an instantiation of its own (the fold-aware one at k = -1 was measured at 1.03x its time).
struct GlmBinomial {
    static constexpr int kVals = kGlmVals;
    static constexpr bool kFold = false, kOffset = false, kWeights = false;
    static constexpr GlmData kData = GlmData::Binomial;
    static constexpr bool kKBeforeOut = false;
    static constexpr const char* kOutNull = "out3 is NULL";
    using Row = GlmRow;
    static __device__ __forceinline__ Row row(double label, double yw, double r, double, double wmin, double) {
        return glm_row(label, yw, r, wmin);
    }
    static __device__ __forceinline__ void add(double* acc, const Row& o, double, double, double, bool, bool, bool train) {
        acc[0] += train ? o.nll : 0.0;
        acc[1] += train ? o.w : 0.0;
        acc[2] += (train && o.clamped) ? 1.0 : 0.0;
    }
    static int32_t refuse_observations(cdh_handle h) {
        if (!h->glm.set) return fail(h, CDH_BAD_ARG, "cdh_glm_irls needs labels: call cdh_glm_set_labels first");
        if (h->glm.family != kData) return fail(h, CDH_BAD_ARG, "the handle holds counts (Poisson): the step is cdh_glm_poisson_irls");
        return CDH_OK;
    }
    static int32_t refuse_params(cdh_handle h, const GlmParams& pm) {
        if (!(pm.wmin > 0.0 && pm.wmin <= 0.25)) return fail(h, CDH_BAD_ARG, "need 0 < wmin <= 0.25");
        return CDH_OK;
    }
};

// The binomial step of a cross-validated path (cv_path.hpp: a fold is a 0/1 observation weight on the resident X; the solves are
// LassoPath's, lasso.jl:229-260, on the weighted loss).  The nll of a held-out row and its misclassification at the current
// iterate (label [eta <= 0] + (1 - label) [eta > 0]: eta = 0 predicts class 0) go into sums of their own: the record is (nll
// of training rows, sum w, clamped training rows, nll of held-out rows, held-out rows misclassified).  The first three are
// GlmBinomial's additions in its order, so with no fold (k < 0) w, y, r and those sums are the plain step's bit for bit and
// the last two are zero.
struct GlmBinomialFold : GlmBinomial {
    static constexpr int kVals = kGlmFoldVals;
    static constexpr bool kFold = true;
    static constexpr const char* kOutNull = "out5 is NULL";
    static __device__ __forceinline__ void add(double* acc, const Row& o, double label, double eta, double v, bool live, bool held,
                                               bool train) {
        GlmBinomial::add(acc, o, label, eta, v, live, held, train);
        acc[3] += held ? o.nll : 0.0;
        acc[4] += held ? (eta > 0.0 ? 1.0 - label : label) : 0.0;
    }
};

// The binomial step of a handle with observation weights (cdh_glm_set_weights): GlmBinomialFold's record with every sum but
// the count of clamped rows weighted by v -- (sum v nll and sum w = sum v w_fam of the training rows, clamped training rows,
// sum v nll and sum v miss of the held-out rows), each product rounded on its own.  It serves cdh_glm_irls too (k = -1, the
// first three sums returned): with weights there is no fold-free instantiation.
struct GlmBinomialFoldW : GlmBinomialFold {
    static constexpr bool kWeights = true;
    static __device__ __forceinline__ void add(double* acc, const Row& o, double label, double eta, double v, bool, bool held,
                                               bool train) {
#pragma clang fp contract(off)
        const double vn = v * o.nll;
        const double vm = v * (eta > 0.0 ? 1.0 - label : label);
        acc[0] += train ? vn : 0.0;
        acc[1] += train ? o.w : 0.0;
        acc[2] += (train && o.clamped) ? 1.0 : 0.0;
        acc[3] += held ? vn : 0.0;
        acc[4] += held ? vm : 0.0;
    }
};

// The Poisson step: fold byte and offset (nullptr: zero; eta_lin + 0.0 makes a null offset and an all-zero one the same bits).
// The record is (nll of training rows, sum w, training rows clamped at wmin, live rows capped at eta_max, deviance of held-out
// rows, deviance of training rows).  57 bytes a row with APPLY (four vectors and a byte read, three vectors written) against
// the fold-aware binomial step's 49.
struct GlmPoisson {
    static constexpr int kVals = kGlmPoisVals;
    static constexpr bool kFold = true, kOffset = true, kWeights = false;
    static constexpr GlmData kData = GlmData::Poisson;
    static constexpr bool kKBeforeOut = true;
    static constexpr const char* kOutNull = "out6 is NULL";
    using Row = PoisRow;
    static __device__ __forceinline__ Row row(double count, double yw, double r, double off, double wmin, double eta_max) {
        return pois_row(count, yw, r, off, wmin, eta_max);
    }
    static __device__ __forceinline__ void add(double* acc, const Row& o, double, double, double, bool live, bool held, bool train) {
        acc[0] += train ? o.nll : 0.0;
        acc[1] += train ? o.w : 0.0;
        acc[2] += (train && o.clamped) ? 1.0 : 0.0;
        acc[3] += (live && o.capped) ? 1.0 : 0.0;
        acc[4] += held ? o.dev : 0.0;
        acc[5] += train ? o.dev : 0.0;
    }
    static int32_t refuse_observations(cdh_handle h) {
        if (!h->glm.set || h->glm.family != kData)
            return fail(h, CDH_BAD_ARG, "cdh_glm_poisson_irls needs counts: call cdh_glm_set_counts first");
        return CDH_OK;
    }
    static int32_t refuse_params(cdh_handle h, const GlmParams& pm) {
        if (!(pm.wmin > 0.0 && pm.wmin <= DBL_MAX)) return fail(h, CDH_BAD_ARG, "need a finite wmin > 0");
        if (!(pm.eta_max > 0.0 && pm.eta_max <= 700.0)) return fail(h, CDH_BAD_ARG, "need 0 < eta_max <= 700");
        return CDH_OK;
    }
};

// The Poisson step of a handle with observation weights: GlmPoisson's record with the nll, sum w = sum v w_fam and both
// deviances weighted by v, each product rounded on its own; clamped and capped stay row counts.  65 bytes a row with APPLY
// (five vectors and a byte read, three vectors written) against GlmPoisson's 57.
struct GlmPoissonW : GlmPoisson {
    static constexpr bool kWeights = true;
    static __device__ __forceinline__ void add(double* acc, const Row& o, double, double, double v, bool live, bool held, bool train) {
#pragma clang fp contract(off)
        const double vn = v * o.nll;
        const double vd = v * o.dev;
        acc[0] += train ? vn : 0.0;
        acc[1] += train ? o.w : 0.0;
        acc[2] += (train && o.clamped) ? 1.0 : 0.0;
        acc[3] += (live && o.capped) ? 1.0 : 0.0;
        acc[4] += held ? vd : 0.0;
        acc[5] += train ? vd : 0.0;
    }
};

// w = v w_fam of a row with an observation weight: one rounded multiplication, after r_new = d / w_fam -- so r and z are the
// unweighted step's bits and X'W r = X'(v (y - mu)) whatever the clamp did to w_fam
__device__ __forceinline__ double glm_prior_times(double v, double w_fam) {
#pragma clang fp contract(off)
    return v * w_fam;
}

// Workgroup b walks tiles b, b + gridDim.x, ... of kGlmRows rows; a lane holds one 16-byte vector of each stream per trip: the
// observations, y, r and -- F::kOffset -- the offset.  A training row becomes (w, z, r_new) of F::row.  A held-out row
// (F::kFold, fold_i == k) gets w = 0 exactly (never clamped up to wmin), z = eta_lin = y - r (X beta, without the offset) and
// r = 0: its row of X enters no gradient, and eta_lin stays recoverable from the two stored vectors after the solver's
// residual updates, so the next step finds its linear predictor where it finds everybody's.  Rows n .. ld - 1 (the pad rows
// every other kernel relies on being zero) are WRITTEN as zeros in w, y and r with APPLY and add nothing to
// the sums -- eta = 0 there would otherwise give w = 0.25, or 1.  The fold id of a row is one byte, n of them, not ld.  A
// lane's vector covers two rows and the last one may lie at or beyond n: the id's address is clamped to n - 1 and the load
// unconditional (as k_path_sse's), so no byte at or beyond n is read; `live` keeps such a row out of everything.  (Measured
// and dropped: both ids in one 2-byte load where both rows lie below n, the clamped byte load elsewhere -- 1.12x the plain
// step against 1.08x for the two byte loads, interleaved at n = 1e7.)  fold == nullptr or k < 0, and offset == nullptr, are
// uniform over the launch.  F::kWeights: `prior` holds ld observation weights, its pad rows zero, so its vector is loaded
// like the observations'; without kWeights the pointer is not looked at.  The lanes' sums go through block_sum (wave butterflies, the four waves in order) into the
// workgroup's record partials[b F::kVals + i]; k_gram_reduce adds the records in block order.  No atomics: bit-identical run
// to run.  With APPLY = false nothing is written but the record.
template <class F, bool APPLY>
__global__ __launch_bounds__(kGlmBlock) void k_glm_step(const double* __restrict__ obs, double* __restrict__ y,
                                                        double* __restrict__ r, double* __restrict__ w,
                                                        const double* __restrict__ offset, const double* __restrict__ prior,
                                                        const uint8_t* __restrict__ fold, int k, int64_t n, int64_t vecs, double wmin, double eta_max,
                                                        double* __restrict__ partials) {
    __shared__ double s_red[F::kVals * (kGlmBlock / 64)];
    const dvec2* bv = reinterpret_cast<const dvec2*>(obs);
    const dvec2* ov = reinterpret_cast<const dvec2*>(offset);
    dvec2* yv = reinterpret_cast<dvec2*>(y);
    dvec2* rv = reinterpret_cast<dvec2*>(r);
    dvec2* wv = reinterpret_cast<dvec2*>(w);
    const bool folded = F::kFold && fold != nullptr && k >= 0;
    const bool has_off = F::kOffset && offset != nullptr;
    double acc[F::kVals] = {};
    const int64_t stride = (int64_t)gridDim.x * kGlmBlock;
    for (int64_t j = (int64_t)blockIdx.x * kGlmBlock + threadIdx.x; j < vecs; j += stride) {
        const dvec2 bb = bv[j], yy = yv[j], rr = rv[j];
        dvec2 oo;
        if (has_off) oo = ov[j]; else { oo[0] = 0.0; oo[1] = 0.0; }
        dvec2 vv;
        if constexpr (F::kWeights) vv = reinterpret_cast<const dvec2*>(prior)[j]; else { vv[0] = 1.0; vv[1] = 1.0; }
        int id[kGlmVec];
#pragma unroll
        for (int e = 0; e < kGlmVec; ++e) {
            const int64_t i = j * kGlmVec + e;
            id[e] = folded ? (int)fold[i < n ? i : n - 1] : -1;
        }
        dvec2 wn, zn, rn;
#pragma unroll
        for (int e = 0; e < kGlmVec; ++e) {
            const bool live = j * kGlmVec + e < n;
            const bool held = live && folded && id[e] == k;
            const bool train = live && !held;
            typename F::Row o = F::row(bb[e], yy[e], rr[e], oo[e], wmin, eta_max);
            if constexpr (F::kWeights) o.w = glm_prior_times(vv[e], o.w);
            const double eta_lin = yy[e] - rr[e];            // (the row functions' own first line)
            wn[e] = train ? o.w : 0.0;
            zn[e] = train ? o.z : (held ? eta_lin : 0.0);
            rn[e] = train ? o.r : 0.0;
            F::add(acc, o, bb[e], eta_lin, vv[e], live, held, train);
        }
        if constexpr (APPLY) { wv[j] = wn; yv[j] = zn; rv[j] = rn; }
    }
    block_sum<F::kVals>(acc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < F::kVals; ++i) partials[(int64_t)blockIdx.x * F::kVals + i] = acc[i];
    }
}
static_assert(kGlmBlock == kBlock && kGlmVec == VecOf<double>::N, "block_sum and dvec2 are kernels.hpp's");

// what every export refuses of the handle itself, before anything is touched (the style of vc_refuse_shards)
int32_t glm_refuse(cdh_handle h) {
    if (h->n != h->n_total || h->xs.sharded())
        return fail(h, CDH_BAD_ARG, "the logistic loss does not run on row-sharded handles");
    if (h->dtype != CDH_F64) return fail(h, CDH_BAD_ARG, "the logistic loss needs fp64 storage (CDH_F64)");
    if (h->loss != CDH_WLS) return fail(h, CDH_BAD_ARG, "the logistic loss needs the CDH_WLS loss");
    return CDH_OK;
}

// cdh_glm_set_labels and cdh_glm_set_counts: leaves the handle exactly as cdh_set_y of n zeros would (what that export voids
// is voided here, in its order), the observations -- labels in [0, 1], or counts that are finite and >= 0, not necessarily
// integers -- and the finite offsets of the Poisson family kept beside it.  Both buffers hold ld doubles, their pad rows
// zero, and are complete before the handle changes.
int32_t glm_set_observations(cdh_handle h, GlmData family, const void* host_obs, const void* host_offset) {
    const bool counts = family == GlmData::Poisson;
    CHK(glm_refuse(h));
    if (!host_obs) return fail(h, CDH_BAD_ARG, counts ? "host_counts is NULL" : "host_labels is NULL");
    const double* obs = (const double*)host_obs;
    const double* off = (const double*)host_offset;
    char buf[128];
    for (int64_t i = 0; i < h->n; ++i)
        if (!(obs[i] >= 0.0 && obs[i] <= (counts ? DBL_MAX : 1.0))) {      // (a NaN fails both comparisons)
            snprintf(buf, sizeof buf, counts ? "counts[%lld] = %g is negative or not finite" : "labels[%lld] = %g is outside [0, 1]",
                     (long long)i, obs[i]);
            return fail(h, CDH_BAD_ARG, buf);
        }
    for (int64_t i = 0; off && i < h->n; ++i)
        if (!(fabs(off[i]) <= DBL_MAX)) {
            snprintf(buf, sizeof buf, "offset[%lld] = %g is not finite", (long long)i, off[i]);
            return fail(h, CDH_BAD_ARG, buf);
        }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t colbytes = (size_t)h->ld * sizeof(double);
    DevBuf<double> fresh, fresh_off;     // complete before the handle changes: a failed allocation leaves it as it was
    if (!h->glm.labels) {
        HIPCHK(h, fresh.alloc(colbytes));
        HIPCHK(h, hipMemsetAsync(fresh, 0, colbytes, h->stream));
    }
    if (off && !h->glm.offset) {
        HIPCHK(h, fresh_off.alloc(colbytes));
        HIPCHK(h, hipMemsetAsync(fresh_off, 0, colbytes, h->stream));
    }
    h->rs.overwritten_with_y();          // r = copy(y) = 0 below
    gc_invalidate(h, false);
    h->gc.st.yy_void();
    h->small.c_valid = false;
    if (!h->glm.labels) h->glm.labels = std::move(fresh);
    if (off && !h->glm.offset) h->glm.offset = std::move(fresh_off);
    HIPCHK(h, hipMemcpyAsync(h->glm.labels, obs, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (off) HIPCHK(h, hipMemcpyAsync(h->glm.offset, off, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->y, 0, colbytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->r, 0, colbytes, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->y_set = true;
    h->glm.family = family;
    h->glm.has_offset = off != nullptr;  // (a Poisson handle turned binomial drops its offset)
    h->glm.cox.strata = false;           // (and a Cox handle its strata and observation weights,
    h->glm.cox.interval = false;         //  its start times
    h->glm.cox.efron = false;            //  and its tie rule)
    h->glm.weighted = false;             // (and every handle the weights of cdh_glm_set_weights)
    h->glm.set = true;
    return CDH_OK;
}

// cdh_glm_set_labels: its family argument stays closed (the Poisson family came in through an export of its own)
int32_t glm_set_labels(cdh_handle h, int32_t family, const void* host_labels) {
    if (family != 0) return fail(h, CDH_BAD_ARG, "unknown family: 0 (binomial) is the only one");
    return glm_set_observations(h, GlmData::Binomial, host_labels, nullptr);
}

// zeros when the counts, or the survival data, came without an offset
int32_t glm_get_offset(cdh_handle h, void* host_offset) {
    NEED_P(h, host_offset);
    if (!h->glm.set || h->glm.family == GlmData::Binomial)      // (a Cox handle keeps its offset in the same buffer)
        return fail(h, CDH_BAD_ARG, "no counts are set: call cdh_glm_set_counts first");
    if (!h->glm.has_offset) {
        memset(host_offset, 0, (size_t)h->n * sizeof(double));
        return CDH_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(host_offset, h->glm.offset, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

int32_t glm_get_labels(cdh_handle h, void* host_labels) {
    NEED_P(h, host_labels);
    if (!h->glm.set) return fail(h, CDH_BAD_ARG, "no labels are set: call cdh_glm_set_labels first");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(host_labels, h->glm.labels, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// cdh_glm_set_weights: the observation weights v of a binomial or a Poisson handle, stored as given in a buffer of ld doubles
// whose pad rows are zero, complete before the handle changes; nullptr drops them.  voids(): what cdh_set_obs_weights voids,
// through its own call (the loss of every later round changes); y, r and beta stay.
template <class Voids>
int32_t glm_set_weights(cdh_handle h, const void* host_weights, Voids&& voids) {
    CHK(glm_refuse(h));
    if (!h->glm.set) return fail(h, CDH_BAD_ARG, "cdh_glm_set_weights needs labels or counts: call cdh_glm_set_labels or cdh_glm_set_counts first");
    if (h->glm.family == GlmData::Cox)
        return fail(h, CDH_BAD_ARG, "the handle holds survival data (Cox): its weights come through cdh_glm_set_survival_strata");
    const double* v = (const double*)host_weights;
    if (v) {
        const int64_t bad = glm_first_bad_weight(v, h->n);
        if (bad < h->n) {
            char buf[128];
            snprintf(buf, sizeof buf, "weights[%lld] = %g is not finite and > 0", (long long)bad, v[bad]);
            return fail(h, CDH_BAD_ARG, buf);
        }
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t colbytes = (size_t)h->ld * sizeof(double);
    DevBuf<double> fresh;                // complete before the handle changes: a failed allocation leaves it as it was
    if (v && !h->glm.prior) {
        HIPCHK(h, fresh.alloc(colbytes));
        HIPCHK(h, hipMemsetAsync(fresh, 0, colbytes, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    CHK(voids());
    if (!v) {
        h->glm.weighted = false;
        return CDH_OK;
    }
    if (!h->glm.prior) h->glm.prior = std::move(fresh);
    h->glm.weighted = false;             // (a failed copy leaves a handle without weights, not one with half of them)
    HIPCHK(h, hipMemcpyAsync(h->glm.prior, v, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->glm.weighted = true;
    return CDH_OK;
}

// ones when the handle holds none
int32_t glm_get_weights(cdh_handle h, void* host_weights) {
    NEED_P(h, host_weights);
    if (!h->glm.set) return fail(h, CDH_BAD_ARG, "no labels or counts are set: call cdh_glm_set_labels or cdh_glm_set_counts first");
    if (h->glm.family == GlmData::Cox)
        return fail(h, CDH_BAD_ARG, "the handle holds survival data (Cox): its weights are cdh_glm_get_survival_strata's");
    if (!h->glm.weighted) {
        std::fill_n((double*)host_weights, (size_t)h->n, 1.0);
        return CDH_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(host_weights, h->glm.prior, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// of k what cdh_set_fold_weights refuses
int32_t glm_refuse_k(cdh_handle h, int32_t k) {
    if (k < -1) return fail(h, CDH_BAD_ARG, "k must be a fold, or -1 for all ones");
    if (k >= 0 && h->cv.K == 0) return fail(h, CDH_BAD_ARG, "k >= 0 needs cdh_set_folds first");
    if (k >= h->cv.K && k >= 0) return fail(h, CDH_BAD_ARG, "k must be below the K of cdh_set_folds");
    return CDH_OK;
}

// what a step's export refuses, before the handle is touched, in the order every export has refused it (the Poisson one
// looks at k before its output pointer, the fold one after: kKBeforeOut)
template <class F>
int32_t glm_check(cdh_handle h, int32_t k, int32_t apply, const GlmParams& pm, const double* out) {
    CHK(glm_refuse(h));
    CHK(F::refuse_observations(h));
    if (apply != 0 && apply != 1) return fail(h, CDH_BAD_ARG, "apply must be 0 or 1");
    CHK(F::refuse_params(h, pm));
    if (F::kFold && F::kKBeforeOut) CHK(glm_refuse_k(h, k));
    if (!out) return fail(h, CDH_BAD_ARG, F::kOutNull);
    if (F::kFold && !F::kKBeforeOut) CHK(glm_refuse_k(h, k));
    if ((size_t)(glm_plan(h->ld, h->knobs.glm_grid).records * F::kVals) > h->sz.partials_doubles)
        return fail(h, CDH_BAD_ARG, "partials too small");
    return CDH_OK;
}

// eta = y - r holds of the residual the handle STANDS FOR at its iterate: r first catches up with what it owes, as for every
// reader of r (cdh_loadings' catch-up); a residual that is not its iterate's is rebuilt through the body cdh_initialize runs
int32_t glm_catch_up(cdh_handle h) {
    if (!h->rs.consistent()) return rebuild_residual(h);
    return sync_r(h);
}

// the pass and its sums: out holds the F::kVals doubles of the family's record, added over the workgroups in block order;
// k = -1: no row is held out and the fold ids are not read
template <class F>
int32_t glm_launch(cdh_handle h, int32_t k, bool apply, const GlmParams& pm, double* out) {
    const GlmPlan pl = glm_plan(h->ld, h->knobs.glm_grid);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid), dim3(kGlmBlock), 0, h->stream, (const double*)h->glm.labels,
                           (double*)h->y, (double*)h->r, (double*)h->w,
                           F::kOffset && h->glm.has_offset ? (const double*)h->glm.offset : (const double*)nullptr,
                           F::kWeights ? (const double*)h->glm.prior : (const double*)nullptr,
                           F::kFold && k >= 0 ? (const uint8_t*)h->cv.fold : (const uint8_t*)nullptr, (int)k, h->n, pl.vecs, pm.wmin,
                           pm.eta_max, (double*)h->d_partials);
    };
    if (apply) go(k_glm_step<F, true>); else go(k_glm_step<F, false>);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_gram_reduce, dim3((F::kVals + kReduceVals - 1) / kReduceVals), dim3(64 * kReduceWaves), 0, h->stream,
                       (const double*)h->d_partials, (int)pl.records, (int)F::kVals, (double*)h->d_red);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_red, sizeof(double) * F::kVals, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}
