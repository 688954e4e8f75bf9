// glm_kernels.hpp -- the step between two rounds of IRLS for l1-penalised logistic regression (no reference counterpart; a
// round's solve is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194): from the linear predictor
// the handle's residual stands for, the working weights, the working response and the new residual in one pass over the
// rows, with the sums a caller needs of it.  Included by cdhip.hip inside its anonymous namespace, after the handle; the
// grid and the rows of a workgroup are glm_plan.hpp's.  The Poisson family with an offset (k_glm_poisson, further down) is
// the same pass with its own row function and record.

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

// Workgroup b walks tiles b, b + gridDim.x, ... of kGlmRows rows; a lane holds one 16-byte vector of each of the three
// streams per trip.  Rows n .. ld - 1 (the pad rows every other kernel relies on being zero) are WRITTEN as
// zeros in w, y and r with APPLY and add nothing to the sums -- eta = 0 there would otherwise give w = 0.25.  The lanes'
// sums go through block_sum (wave butterflies, the four waves in order) into the workgroup's record
// partials[b kGlmVals + {0, 1, 2}] = (sum nll, sum w, clamped rows); k_gram_reduce adds the records in block order.  No
// atomics: bit-identical run to run.  With APPLY = false nothing is written but the record.
template <bool APPLY>
__global__ __launch_bounds__(kGlmBlock) void k_glm_irls(const double* __restrict__ label, double* __restrict__ y,
                                                        double* __restrict__ r, double* __restrict__ w, int64_t n,
                                                        int64_t vecs, double wmin, double* __restrict__ partials) {
    __shared__ double s_red[kGlmVals * (kGlmBlock / 64)];
    const dvec2* lv = reinterpret_cast<const dvec2*>(label);
    dvec2* yv = reinterpret_cast<dvec2*>(y);
    dvec2* rv = reinterpret_cast<dvec2*>(r);
    dvec2* wv = reinterpret_cast<dvec2*>(w);
    double acc[kGlmVals] = {0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kGlmBlock;
    for (int64_t j = (int64_t)blockIdx.x * kGlmBlock + threadIdx.x; j < vecs; j += stride) {
        const dvec2 ll = lv[j], yy = yv[j], rr = rv[j];
        dvec2 wn, zn, rn;
#pragma unroll
        for (int e = 0; e < kGlmVec; ++e) {
            const bool live = j * kGlmVec + e < n;
            const GlmRow o = glm_row(ll[e], yy[e], rr[e], wmin);
            wn[e] = live ? o.w : 0.0;
            zn[e] = live ? o.z : 0.0;
            rn[e] = live ? o.r : 0.0;
            acc[0] += live ? o.nll : 0.0;
            acc[1] += live ? o.w : 0.0;
            acc[2] += (live && o.clamped) ? 1.0 : 0.0;
        }
        if constexpr (APPLY) { wv[j] = wn; yv[j] = zn; rv[j] = rn; }
    }
    block_sum<kGlmVals>(acc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kGlmVals; ++i) partials[(int64_t)blockIdx.x * kGlmVals + i] = acc[i];
    }
}
static_assert(kGlmBlock == kBlock && kGlmVec == VecOf<double>::N, "block_sum and dvec2 are kernels.hpp's");

// The step of a cross-validated path (cv_path.hpp: a fold is a 0/1 observation weight on the resident X; the solves are
// LassoPath's, lasso.jl:229-260, on the weighted loss): k_glm_irls' grid, tiles, vectors and sums, with the fold id of every
// row -- one byte, n of them, not ld -- deciding what the row becomes.  A training row (fold_i != k) is k_glm_irls' row.  A
// held-out row (fold_i == k) gets w = 0 exactly (never clamped up to wmin), z = eta and r = 0: its row of X enters no
// gradient, and eta = y - r stays recoverable from the two stored vectors after the solver's residual updates, so the next
// step finds its linear predictor where it finds everybody's.  Its nll and its misclassification at the current iterate
// (label [eta <= 0] + (1 - label) [eta > 0]: eta = 0 predicts class 0) go into sums of their own.  The record is
// partials[b kGlmFoldVals + {0 .. 4}] = (nll of training rows, sum w, clamped training rows, nll of held-out rows, held-out
// rows misclassified); lane sums, block_sum and k_gram_reduce take every value in k_glm_irls' order, so with no fold
// (fold == nullptr or k < 0) w, y, r and the first three sums are k_glm_irls' bit for bit and the last two are zero.
// A lane's vector covers two rows and the last one may lie at or beyond n: the id's address is clamped to n - 1 and the load
// unconditional (as k_path_sse's), so no byte at or beyond n is read; `live` keeps such a row out of everything.  (Measured
// and dropped: both ids in one 2-byte load where both rows lie below n, the clamped byte load elsewhere -- 1.12x the plain
// step against 1.08x for the two byte loads, interleaved at n = 1e7.)
template <bool APPLY>
__global__ __launch_bounds__(kGlmBlock) void k_glm_irls_fold(const double* __restrict__ label, double* __restrict__ y,
                                                             double* __restrict__ r, double* __restrict__ w,
                                                             const uint8_t* __restrict__ fold, int k, int64_t n,
                                                             int64_t vecs, double wmin, double* __restrict__ partials) {
    __shared__ double s_red[kGlmFoldVals * (kGlmBlock / 64)];
    const dvec2* lv = reinterpret_cast<const dvec2*>(label);
    dvec2* yv = reinterpret_cast<dvec2*>(y);
    dvec2* rv = reinterpret_cast<dvec2*>(r);
    dvec2* wv = reinterpret_cast<dvec2*>(w);
    const bool folded = fold != nullptr && k >= 0;           // (uniform over the launch)
    double acc[kGlmFoldVals] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kGlmBlock;
    for (int64_t j = (int64_t)blockIdx.x * kGlmBlock + threadIdx.x; j < vecs; j += stride) {
        const dvec2 ll = lv[j], yy = yv[j], rr = rv[j];
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
            const GlmRow o = glm_row(ll[e], yy[e], rr[e], wmin);
            const double eta = yy[e] - rr[e];                // (glm_row's own first line)
            wn[e] = train ? o.w : 0.0;
            zn[e] = train ? o.z : (held ? eta : 0.0);
            rn[e] = train ? o.r : 0.0;
            acc[0] += train ? o.nll : 0.0;
            acc[1] += train ? o.w : 0.0;
            acc[2] += (train && o.clamped) ? 1.0 : 0.0;
            acc[3] += held ? o.nll : 0.0;
            acc[4] += held ? (eta > 0.0 ? 1.0 - ll[e] : ll[e]) : 0.0;
        }
        if constexpr (APPLY) { wv[j] = wn; yv[j] = zn; rv[j] = rn; }
    }
    block_sum<kGlmFoldVals>(acc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kGlmFoldVals; ++i) partials[(int64_t)blockIdx.x * kGlmFoldVals + i] = acc[i];
    }
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

// k_glm_irls_fold's grid, tiles, vectors, block_sum and k_gram_reduce with a fourth 16-byte stream, the offset (nullptr: zero;
// the branch is uniform over the launch, and eta_lin + 0.0 makes a null offset and an all-zero one the same bits).  A training
// row becomes (w, z_lin, r_new); a held-out row (fold_i == k) becomes (0, eta_lin, 0) -- weight exactly zero, never clamped up --
// and its deviance at the current iterate goes into a sum of its own; rows n .. ld - 1 are WRITTEN as zeros and add to no sum
// (eta = 0 there would otherwise give w = 1).  The fold byte is read for n rows, not ld: the address is clamped to n - 1 as in
// k_glm_irls_fold.  The record is partials[b kGlmPoisVals + {0 .. 5}] = (nll of training rows, sum w, training rows clamped at
// wmin, live rows capped at eta_max, deviance of held-out rows, deviance of training rows).  No atomics: bit-identical run to
// run.  With APPLY = false nothing is written but the record.  57 bytes a row with APPLY (four vectors and a byte read, three
// vectors written) against the fold-aware binomial step's 49.
template <bool APPLY>
__global__ __launch_bounds__(kGlmBlock) void k_glm_poisson(const double* __restrict__ count, double* __restrict__ y,
                                                           double* __restrict__ r, double* __restrict__ w,
                                                           const double* __restrict__ offset, const uint8_t* __restrict__ fold,
                                                           int k, int64_t n, int64_t vecs, double wmin, double eta_max,
                                                           double* __restrict__ partials) {
    __shared__ double s_red[kGlmPoisVals * (kGlmBlock / 64)];
    const dvec2* cv = reinterpret_cast<const dvec2*>(count);
    const dvec2* ov = reinterpret_cast<const dvec2*>(offset);
    dvec2* yv = reinterpret_cast<dvec2*>(y);
    dvec2* rv = reinterpret_cast<dvec2*>(r);
    dvec2* wv = reinterpret_cast<dvec2*>(w);
    const bool folded = fold != nullptr && k >= 0;           // (uniform over the launch)
    const bool has_off = offset != nullptr;                  // (uniform over the launch)
    double acc[kGlmPoisVals] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kGlmBlock;
    for (int64_t j = (int64_t)blockIdx.x * kGlmBlock + threadIdx.x; j < vecs; j += stride) {
        const dvec2 cc = cv[j], yy = yv[j], rr = rv[j];
        dvec2 oo;
        if (has_off) oo = ov[j]; else { oo[0] = 0.0; oo[1] = 0.0; }
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
            const PoisRow o = pois_row(cc[e], yy[e], rr[e], oo[e], wmin, eta_max);
            wn[e] = train ? o.w : 0.0;
            zn[e] = train ? o.z : (held ? o.eta_lin : 0.0);
            rn[e] = train ? o.r : 0.0;
            acc[0] += train ? o.nll : 0.0;
            acc[1] += train ? o.w : 0.0;
            acc[2] += (train && o.clamped) ? 1.0 : 0.0;
            acc[3] += (live && o.capped) ? 1.0 : 0.0;
            acc[4] += held ? o.dev : 0.0;
            acc[5] += train ? o.dev : 0.0;
        }
        if constexpr (APPLY) { wv[j] = wn; yv[j] = zn; rv[j] = rn; }
    }
    block_sum<kGlmPoisVals>(acc, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kGlmPoisVals; ++i) partials[(int64_t)blockIdx.x * kGlmPoisVals + i] = acc[i];
    }
}

// what the three exports refuse of the handle itself, before anything is touched (the style of vc_refuse_shards)
int32_t glm_refuse(cdh_handle h) {
    if (h->n != h->n_total || h->xs.sharded())
        return fail(h, CDH_BAD_ARG, "the logistic loss does not run on row-sharded handles");
    if (h->dtype != CDH_F64) return fail(h, CDH_BAD_ARG, "the logistic loss needs fp64 storage (CDH_F64)");
    if (h->loss != CDH_WLS) return fail(h, CDH_BAD_ARG, "the logistic loss needs the CDH_WLS loss");
    return CDH_OK;
}

// leaves the handle exactly as cdh_set_y of n zeros would (what that export voids is voided here, in its order)
int32_t glm_set_labels(cdh_handle h, int32_t family, const void* host_labels) {
    if (family != 0) return fail(h, CDH_BAD_ARG, "unknown family: 0 (binomial) is the only one");
    CHK(glm_refuse(h));
    NEED_P(h, host_labels);
    const double* lab = (const double*)host_labels;
    for (int64_t i = 0; i < h->n; ++i)
        if (!(lab[i] >= 0.0 && lab[i] <= 1.0)) {      // (a NaN fails both comparisons)
            char buf[128];
            snprintf(buf, sizeof buf, "labels[%lld] = %g is outside [0, 1]", (long long)i, lab[i]);
            return fail(h, CDH_BAD_ARG, buf);
        }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t colbytes = (size_t)h->ld * sizeof(double);
    DevBuf<double> fresh;                // complete before the handle changes: a failed allocation leaves it as it was
    if (!h->glm.labels) {
        HIPCHK(h, fresh.alloc(colbytes));
        HIPCHK(h, hipMemsetAsync(fresh, 0, colbytes, h->stream));
    }
    h->rs.overwritten_with_y();          // r = copy(y) = 0 below
    gc_invalidate(h, false);
    h->gc.st.yy_void();
    h->small.c_valid = false;
    if (!h->glm.labels) h->glm.labels = std::move(fresh);
    HIPCHK(h, hipMemcpyAsync(h->glm.labels, lab, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->y, 0, colbytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->r, 0, colbytes, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->y_set = true;
    h->glm.family = family;
    h->glm.has_offset = false;           // (a Poisson handle turned binomial drops its offset)
    h->glm.set = true;
    return CDH_OK;
}

// cdh_glm_set_counts: glm_set_labels for the Poisson family (family 1), the offset kept beside the counts.  Counts are finite
// and >= 0 (not necessarily integers), offsets finite; both buffers are complete before the handle changes, and what is
// voided is what glm_set_labels voids, in its order.  The offset buffer holds ld doubles, its pad rows zero.
int32_t glm_set_counts(cdh_handle h, const void* host_counts, const void* host_offset) {
    CHK(glm_refuse(h));
    NEED_P(h, host_counts);
    const double* cnt = (const double*)host_counts;
    const double* off = (const double*)host_offset;
    for (int64_t i = 0; i < h->n; ++i)
        if (!(cnt[i] >= 0.0 && cnt[i] <= DBL_MAX)) {      // (a NaN fails both comparisons)
            char buf[128];
            snprintf(buf, sizeof buf, "counts[%lld] = %g is negative or not finite", (long long)i, cnt[i]);
            return fail(h, CDH_BAD_ARG, buf);
        }
    for (int64_t i = 0; off && i < h->n; ++i)
        if (!(fabs(off[i]) <= DBL_MAX)) {
            char buf[128];
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
    HIPCHK(h, hipMemcpyAsync(h->glm.labels, cnt, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (off) HIPCHK(h, hipMemcpyAsync(h->glm.offset, off, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->y, 0, colbytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->r, 0, colbytes, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->y_set = true;
    h->glm.family = 1;
    h->glm.has_offset = off != nullptr;
    h->glm.set = true;
    return CDH_OK;
}

// zeros when the counts came without an offset
int32_t glm_get_offset(cdh_handle h, void* host_offset) {
    NEED_P(h, host_offset);
    if (!h->glm.set || h->glm.family != 1) return fail(h, CDH_BAD_ARG, "no counts are set: call cdh_glm_set_counts first");
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

// what cdh_glm_irls refuses, before the handle is touched
int32_t glm_check_irls(cdh_handle h, int32_t apply, double wmin, const double* out3) {
    CHK(glm_refuse(h));
    if (!h->glm.set) return fail(h, CDH_BAD_ARG, "cdh_glm_irls needs labels: call cdh_glm_set_labels first");
    if (h->glm.family != 0) return fail(h, CDH_BAD_ARG, "the handle holds counts (Poisson): the step is cdh_glm_poisson_irls");
    if (apply != 0 && apply != 1) return fail(h, CDH_BAD_ARG, "apply must be 0 or 1");
    if (!(wmin > 0.0 && wmin <= 0.25)) return fail(h, CDH_BAD_ARG, "need 0 < wmin <= 0.25");
    NEED_P(h, out3);
    if ((size_t)(glm_plan(h->ld, h->knobs.glm_grid).records * kGlmVals) > h->partials_doubles)
        return fail(h, CDH_BAD_ARG, "partials too small");
    return CDH_OK;
}

// what cdh_glm_irls_fold refuses, before the handle is touched: all of the above, and of k what cdh_set_fold_weights refuses
int32_t glm_check_irls_fold(cdh_handle h, int32_t k, int32_t apply, double wmin, const double* out5) {
    CHK(glm_check_irls(h, apply, wmin, out5));
    if (k < -1) return fail(h, CDH_BAD_ARG, "k must be a fold, or -1 for all ones");
    if (k >= 0 && h->cv.K == 0) return fail(h, CDH_BAD_ARG, "k >= 0 needs cdh_set_folds first");
    if (k >= h->cv.K && k >= 0) return fail(h, CDH_BAD_ARG, "k must be below the K of cdh_set_folds");
    if ((size_t)(glm_plan(h->ld, h->knobs.glm_grid).records * kGlmFoldVals) > h->partials_doubles)
        return fail(h, CDH_BAD_ARG, "partials too small");
    return CDH_OK;
}

// what cdh_glm_poisson_irls refuses, before the handle is touched
int32_t glm_check_poisson(cdh_handle h, int32_t k, int32_t apply, double wmin, double eta_max, const double* out6) {
    CHK(glm_refuse(h));
    if (!h->glm.set || h->glm.family != 1)
        return fail(h, CDH_BAD_ARG, "cdh_glm_poisson_irls needs counts: call cdh_glm_set_counts first");
    if (apply != 0 && apply != 1) return fail(h, CDH_BAD_ARG, "apply must be 0 or 1");
    if (!(wmin > 0.0 && wmin <= DBL_MAX)) return fail(h, CDH_BAD_ARG, "need a finite wmin > 0");
    if (!(eta_max > 0.0 && eta_max <= 700.0)) return fail(h, CDH_BAD_ARG, "need 0 < eta_max <= 700");
    if (k < -1) return fail(h, CDH_BAD_ARG, "k must be a fold, or -1 for all ones");
    if (k >= 0 && h->cv.K == 0) return fail(h, CDH_BAD_ARG, "k >= 0 needs cdh_set_folds first");
    if (k >= h->cv.K && k >= 0) return fail(h, CDH_BAD_ARG, "k must be below the K of cdh_set_folds");
    NEED_P(h, out6);
    if ((size_t)(glm_plan(h->ld, h->knobs.glm_grid).records * kGlmPoisVals) > h->partials_doubles)
        return fail(h, CDH_BAD_ARG, "partials too small");
    return CDH_OK;
}

// eta = y - r holds of the residual the handle STANDS FOR at its iterate: r first catches up with what it owes, as for every
// reader of r (cdh_loadings' catch-up); a residual that is not its iterate's is rebuilt through the body cdh_initialize runs
int32_t glm_catch_up(cdh_handle h) {
    if (!h->rs.consistent()) return rebuild_residual(h);
    return sync_r(h);
}

// the pass and its sums: out3 = (sum nll, sum w, clamped rows)
int32_t glm_launch(cdh_handle h, bool apply, double wmin, double* out3) {
    const GlmPlan pl = glm_plan(h->ld, h->knobs.glm_grid);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid), dim3(kGlmBlock), 0, h->stream, (const double*)h->glm.labels,
                           (double*)h->y, (double*)h->r, (double*)h->w, h->n, pl.vecs, wmin, (double*)h->d_partials);
    };
    if (apply) go(k_glm_irls<true>); else go(k_glm_irls<false>);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_gram_reduce, dim3((kGlmVals + kReduceVals - 1) / kReduceVals), dim3(64 * kReduceWaves), 0, h->stream,
                       (const double*)h->d_partials, (int)pl.records, (int)kGlmVals, (double*)h->d_red);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out3, h->d_red, sizeof(double) * kGlmVals, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// the fold-aware pass and its sums: out5 = (nll of training rows, sum w, clamped rows, nll of held-out rows, held-out rows
// misclassified); k = -1: no row is held out and the fold ids are not read
int32_t glm_launch_fold(cdh_handle h, int32_t k, bool apply, double wmin, double* out5) {
    const GlmPlan pl = glm_plan(h->ld, h->knobs.glm_grid);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid), dim3(kGlmBlock), 0, h->stream, (const double*)h->glm.labels,
                           (double*)h->y, (double*)h->r, (double*)h->w,
                           k >= 0 ? (const uint8_t*)h->cv.fold : (const uint8_t*)nullptr, (int)k, h->n, pl.vecs, wmin,
                           (double*)h->d_partials);
    };
    if (apply) go(k_glm_irls_fold<true>); else go(k_glm_irls_fold<false>);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_gram_reduce, dim3((kGlmFoldVals + kReduceVals - 1) / kReduceVals), dim3(64 * kReduceWaves), 0, h->stream,
                       (const double*)h->d_partials, (int)pl.records, (int)kGlmFoldVals, (double*)h->d_red);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out5, h->d_red, sizeof(double) * kGlmFoldVals, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// the Poisson pass and its sums: out6 = (nll of training rows, sum w, clamped training rows, capped live rows, deviance of
// held-out rows, deviance of training rows); k = -1: no row is held out and the fold ids are not read
int32_t glm_launch_poisson(cdh_handle h, int32_t k, bool apply, double wmin, double eta_max, double* out6) {
    const GlmPlan pl = glm_plan(h->ld, h->knobs.glm_grid);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)pl.grid), dim3(kGlmBlock), 0, h->stream, (const double*)h->glm.labels,
                           (double*)h->y, (double*)h->r, (double*)h->w,
                           h->glm.has_offset ? (const double*)h->glm.offset : (const double*)nullptr,
                           k >= 0 ? (const uint8_t*)h->cv.fold : (const uint8_t*)nullptr, (int)k, h->n, pl.vecs, wmin, eta_max,
                           (double*)h->d_partials);
    };
    if (apply) go(k_glm_poisson<true>); else go(k_glm_poisson<false>);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_gram_reduce, dim3((kGlmPoisVals + kReduceVals - 1) / kReduceVals), dim3(64 * kReduceWaves), 0, h->stream,
                       (const double*)h->d_partials, (int)pl.records, (int)kGlmPoisVals, (double*)h->d_red);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out6, h->d_red, sizeof(double) * kGlmPoisVals, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}
