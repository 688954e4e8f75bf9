// col_stats.hpp -- the bodies of the read-only statistics exports: column scales, loadings and dots, Gram blocks, a row of X, the
// residual's moments, the objective, a coordinate's gradient, lambda_max.  Each is col_dots, col_loadings, resid_moments_dev or
// a Gram launch, one read-back (col_dots.hpp: ColPairs, ResidSums) and host arithmetic; which Gram launches a call makes and
// where their records go is stats_plan.hpp's to say.  Included by cdhip.hip, in its anonymous namespace, behind vc_host.hpp,
// where the last of this code stood (cdh_get_X_row: the first use of k_gather_row, and the place decides the order of the
// kernels in the code object); lambda_max is declared ahead of the solves that call it.

// ---- column scales, loadings, dots ------------------------------------------------------------------------------------------------
int32_t col_rms(cdh_handle h, double* out_p) {
    NEED_P(h, out_p);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(col_dots(h, 0, h->p, h->r, false));
    std::vector<double> cd;
    CHK(read_col_pairs(h, h->p, cd));
    const ColPairs pairs(cd);
    for (int64_t j = 0; j < h->p; ++j) out_p[j] = std::sqrt(pairs.sq(j) / (double)h->n_total);
    return CDH_OK;
}

// _stdX!(out, w, X) (utils.jl:140-151): out_j = sqrt(sum_i w_i X_ij^2 / n_total)
int32_t col_wrms(cdh_handle h, double* out_p) {
    NEED_P(h, out_p);
    if (h->loss != CDH_WLS || !h->has_w) return fail(h, CDH_BAD_ARG, "weighted column scales need the CDH_WLS loss with its weights set");
    HIPCHK(h, hipSetDevice(h->device));
    CHK(col_dots(h, 0, h->p, h->y, true));      // (the dots with y are not used; r may owe updates nobody needs here)
    std::vector<double> cd;
    CHK(read_col_pairs(h, h->p, cd));
    const ColPairs pairs(cd);
    for (int64_t j = 0; j < h->p; ++j) out_p[j] = std::sqrt(pairs.sq(j) / (double)h->n_total);
    return CDH_OK;
}

int32_t loadings(cdh_handle h, double* out_p) {
    NEED_P(h, out_p);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(col_loadings(h));
    HIPCHK(h, hipMemcpyAsync(out_p, h->d_colout, sizeof(double) * h->p, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t j = 0; j < h->p; ++j) out_p[j] = std::sqrt(out_p[j] / (double)h->n_total);
    return CDH_OK;
}

int32_t xt_r(cdh_handle h, double* out_p) {
    NEED_P(h, out_p);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(col_dots(h, 0, h->p, h->r, false));
    std::vector<double> cd;
    CHK(read_col_pairs(h, h->p, cd));
    const ColPairs pairs(cd);
    for (int64_t j = 0; j < h->p; ++j) out_p[j] = pairs.dot(j);
    h->rs.dots_taken(std::move(cd), false);
    return CDH_OK;
}

// X_S'r (X_S'Wr for the weighted loss) for a list of columns: the refinement step of the screening init reads the normal
// equations' residual off it (src/utils.jl:65-77 solves Xs \ y by QR; here: the Gram block plus refinement)
int32_t xt_r_cols(cdh_handle h, int64_t m, const int64_t* idx1, double* out_m) {
    if (m < 1 || m > h->cap) return fail(h, CDH_BAD_ARG, "need 1 <= m <= max(p, 4096) columns");
    NEED_P(h, idx1);
    NEED_P(h, out_m);
    CHK(check_columns(h, idx1, m));
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<double> cd;
    for (int64_t o = 0; o < m; o += h->p) {          // d_colout holds 2p values
        const int64_t mm = std::min<int64_t>(h->p, m - o);
        for (int64_t i = 0; i < mm; ++i) h->h_idx[i] = idx1[o + i] - 1;
        HIPCHK(h, hipMemcpyAsync(h->d_idx, h->h_idx, sizeof(int64_t) * (size_t)mm, hipMemcpyHostToDevice, h->stream));
        CHK(col_dots(h, 0, mm, h->r, h->loss == CDH_WLS, h->d_idx));
        CHK(read_col_pairs(h, mm, cd));
        const ColPairs pairs(cd);
        for (int64_t i = 0; i < mm; ++i) out_m[o + i] = pairs.dot(i);
    }
    return CDH_OK;
}

// wX[i, S] (:132): out_m[k] = X[row0, idx1[k]] of the resident design, as doubles
int32_t get_X_row(cdh_handle h, int64_t row0, int64_t m, const int64_t* idx1, double* out_m) {
    if (m < 1 || m > kGramMaxCols) return fail(h, CDH_BAD_ARG, "need 1 <= m <= 4096 columns");
    NEED_P(h, idx1);
    NEED_P(h, out_m);
    if (row0 < 0 || row0 >= h->n) return fail(h, CDH_BAD_ARG, "row outside 0 .. n_local - 1");
    CHK(check_columns(h, idx1, m));
    HIPCHK(h, hipSetDevice(h->device));
    for (int64_t o = 0; o < m; o += 2 * h->p) {          // d_colout holds 2p values
        const int64_t mm = std::min<int64_t>(2 * h->p, m - o);
        for (int64_t i = 0; i < mm; ++i) h->h_idx[i] = idx1[o + i] - 1;
        HIPCHK(h, hipMemcpyAsync(h->d_idx, h->h_idx, sizeof(int64_t) * (size_t)mm, hipMemcpyHostToDevice, h->stream));
        CHK(dispatch(h, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            hipLaunchKernelGGL(k_gather_row<T>, dim3((unsigned)((mm + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream,
                               (const T*)h->X, h->ld, row0, h->d_idx, (int)mm, h->d_colout);
            return CDH_OK;
        }));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(out_m + o, h->d_colout, sizeof(double) * (size_t)mm, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return CDH_OK;
}

// ---- Gram blocks --------------------------------------------------------------------------------------------------------------------
// one launch of the wide-block Gram kernel over up to 64 columns (0-based, in h->h_idx[0 .. m)): rec <- (G, c = X_S'r, q = r'r);
// with `weighted`, G = X_S'WX_S and c = X_S'Wr (q stays r'r: the kernel weights its A operands only)
int32_t gram_launch(cdh_handle h, int m, std::vector<double>& rec, bool weighted) {
    using R = GramRec<4>;
    HIPCHK(h, hipMemcpyAsync(h->d_idx, h->h_idx, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, h->stream));
    // one k_gramstep launch with no pending update: r is only read
    const int G = gram_read_grid(h->nvec, h->sz.cus);
    CHK(need_partials(h, (size_t)G * R::N, "partial buffer too small for this grid"));
    CHK(dispatch(h, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        hipLaunchKernelGGL((k_gramstep<T, 4>), dim3(G), dim3(64 * kGramWaves), 0, h->stream,
                           (const T*)h->X, h->ld, h->nvec, weighted ? (const T*)h->w : (const T*)nullptr, (T*)h->r, h->d_idx,
                           h->d_hs, 0, m, 0, h->d_partials);
        return CDH_OK;
    }));
    hipLaunchKernelGGL(k_gram_reduce, dim3((R::N + kReduceVals - 1) / kReduceVals), dim3(64 * kReduceWaves), 0, h->stream, h->d_partials, G, R::N, h->d_red);
    HIPCHK(h, hipGetLastError());
    CHK(allreduce(h, h->d_red, R::N));
    rec.resize((size_t)R::N);
    HIPCHK(h, hipMemcpyAsync(rec.data(), h->d_red, sizeof(double) * R::N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}
// the launches of stats_plan.hpp, one after the other: columns up, launch, record down, scatter
int32_t gram_block(cdh_handle h, int64_t m, const int64_t* idx1, double* out_G, double* out_c, double* out_q, bool weighted) {
    if (m < 1 || m > kGramMaxCols) return fail(h, CDH_BAD_ARG, "need 1 <= m <= 4096 columns");
    NEED_P(h, idx1);
    NEED_P(h, out_G);
    CHK(check_columns(h, idx1, m));
    HIPCHK(h, hipSetDevice(h->device));
    CHK(sync_r(h));
    std::vector<double> rec;
    for (int64_t t = 0; t < gram_launches(m); ++t) {
        const GramLaunch L = gram_launch_at(m, t);
        for (int pos = 0; pos < L.cols(); ++pos) h->h_idx[pos] = idx1[L.col_of(pos)] - 1;
        CHK(gram_launch(h, L.cols(), rec, weighted));
        gram_scatter(L, m, rec.data(), out_G, out_c, out_q);
    }
    return CDH_OK;
}

// X_S'WX_S, X_S'Wr, r'Wr: the weighted normal equations of the refit of locpolyl1 (varying_coefficient_lasso.jl:71-76) at the
// current residual.  The Gram kernel weights G and c; r'Wr is the weighted moment of r.
int32_t gram_weighted(cdh_handle h, int64_t m, const int64_t* idx1, double* out_G, double* out_c, double* out_q) {
    if (h->loss != CDH_WLS || !h->has_w) return fail(h, CDH_BAD_ARG, "a weighted Gram block needs the CDH_WLS loss with its weights set");
    CHK(gram_block(h, m, idx1, out_G, out_c, nullptr, true));
    if (out_q) {
        ResidSums s;
        CHK(resid_moments_dev(h));
        CHK(read_resid_sums(h, &s));
        *out_q = s.wsumsq;
    }
    return CDH_OK;
}

// ---- the residual's moments ---------------------------------------------------------------------------------------------------------
int32_t resid_moments(cdh_handle h, double* out_sum, double* out_sumsq) {
    HIPCHK(h, hipSetDevice(h->device));
    ResidSums s;
    CHK(resid_moments_dev(h));
    CHK(read_resid_sums(h, &s));
    if (out_sum) *out_sum = s.sum;
    if (out_sumsq) *out_sumsq = s.sumsq;
    return CDH_OK;
}

// _getSigma(w, r) (utils.jl:167-175): sum w, sum w r^2 at the current residual
int32_t resid_wmoments(cdh_handle h, double* out_sum_w, double* out_sum_wr2) {
    if (h->loss != CDH_WLS || !h->has_w) return fail(h, CDH_BAD_ARG, "weighted moments need the CDH_WLS loss with its weights set");
    HIPCHK(h, hipSetDevice(h->device));
    ResidSums s;
    CHK(resid_moments_dev(h, nullptr, 0.0, true));
    CHK(read_resid_sums(h, &s));
    if (out_sum_w) *out_sum_w = s.sum;
    if (out_sum_wr2) *out_sum_wr2 = s.wsumsq;
    return CDH_OK;
}

// std(f.r) as Statistics.std computes it (two passes: the mean, then the centred sum of squares; Bessel-corrected) --
// lasso.jl:37,52,81,97,143 -- without the cancellation of the one-pass form when the mean is large against the spread
int32_t resid_std(cdh_handle h, double* out_std, double* out_mean) {
    NEED_P(h, out_std);
    HIPCHK(h, hipSetDevice(h->device));
    ResidSums s;
    CHK(resid_moments_dev(h));
    CHK(read_resid_sums(h, &s));
    const double n = (double)h->n_total, mean = s.sum / n;
    double ss = s.sumsq, s1 = 0.0;
    if (mean != 0.0 && mean == mean) {
        CHK(resid_moments_dev(h, nullptr, mean));
        CHK(read_resid_sums(h, &s));
        s1 = s.sum; ss = s.sumsq;         // of the centred values: s1 is rounding-sized
    }
    *out_std = std::sqrt(std::max(ss - s1 * s1 / n, 0.0) / (n - 1.0));
    if (out_mean) *out_mean = mean;
    return CDH_OK;
}

int32_t objective(cdh_handle h, double* out) {
    NEED_P(h, out);
    HIPCHK(h, hipSetDevice(h->device));
    ResidSums s;
    CHK(resid_moments_dev(h));
    CHK(read_resid_sums(h, &s));
    const std::vector<double>& om = h->h_omega;
    double pen = 0.0;
    for (int64_t k = 0; k < h->x.nnz(); ++k)
        pen += std::fabs(h->x.slot_value(k)) * (h->has_omega ? om[(size_t)h->x.coord(k)] : 1.0);
    pen *= h->ctrl.lambda0;
    const double ss = h->loss == CDH_WLS ? s.wsumsq : s.sumsq;
    *out = (h->loss == CDH_SQRT ? std::sqrt(ss) : ss / (2.0 * (double)h->n_total)) + pen;
    return CDH_OK;
}

// ---- a coordinate's gradient, lambda_max --------------------------------------------------------------------------------------------
// (its one pair comes back through the pinned staging block, ahead of the residual's sums)
int32_t gradient(cdh_handle h, int64_t k1, double* out) {
    NEED_P(h, out);
    CHK(check_coordinate(h, k1));
    HIPCHK(h, hipSetDevice(h->device));
    CHK(col_dots(h, k1 - 1, 1, h->r, h->loss == CDH_WLS));
    HIPCHK(h, hipMemcpyAsync(h->h_red, h->d_colout, sizeof(double) * 2, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const double xr = ColPairs(h->h_red).dot(0);
    double denom = (double)h->n_total;
    if (h->loss == CDH_SQRT) {
        ResidSums s;
        CHK(resid_moments_dev(h));
        CHK(read_resid_sums(h, &s));
        denom = std::sqrt(s.sumsq);
    }
    *out = -xr / denom;
    return CDH_OK;
}

int32_t lambda_max(cdh_handle h, double* out, std::vector<double>* dots /* the (X_k'r, a_k) pairs, for a caller that can use them */) {
    CHK(col_dots(h, 0, h->p, h->r, h->loss == CDH_WLS));
    std::vector<double> cd_own;
    std::vector<double>& cd = dots ? *dots : cd_own;
    CHK(queue_col_pairs(h, h->p, cd));
    double denom = (double)h->n_total;
    if (h->loss == CDH_SQRT) {
        CHK(resid_moments_dev(h));
        CHK(queue_resid_sums(h));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->rs.dots_taken(cd, h->loss == CDH_WLS);   // (col_dots has brought r up to date first)
    if (h->loss == CDH_SQRT) denom = std::sqrt(resid_sums(h).sumsq);
    *out = lambda_max_of(cd.data(), 2, h->p, denom, h->has_omega ? h->h_omega.data() : nullptr);   // the dots of the (X_k'r, a_k) pairs
    return CDH_OK;
}
