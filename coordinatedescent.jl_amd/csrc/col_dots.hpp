// col_dots.hpp -- the row-summing launches beside the streamed sweep: col_dots, col_loadings, resid_moments_dev, the one
// bound on the partial records every launcher checks, and the read-back of what the first and the last leave on the device
// (ColPairs, ResidSums: every host site that reads d_colout's pairs or d_red's sums goes through them).  Included by cdhip.hip,
// in its anonymous namespace, where this code has always stood (ahead of rebuild_residual_from: the place decides the order of
// the kernels in the code object).  Row chunks and grids are sweep_plan.hpp's to say.

// the one bound on the workgroups' partial records (cdh_create sized them for every launch the plan can ask for)
inline int32_t need_partials(cdh_handle h, size_t doubles, const char* msg = "partials too small") {
    return doubles > h->sz.partials_doubles ? fail(h, CDH_BAD_ARG, msg) : (int32_t)CDH_OK;
}

// ---- column dots over columns [j0, j0+nc): d_colout[2*j + {0,1}] = (x.r (w), x.x (w)) ----
int32_t col_dots(cdh_handle h, int64_t j0, int64_t nc, const void* rvec, bool use_w,
                 const int64_t* d_cols = nullptr) {
    if (rvec == h->r) CHK(sync_r(h));
    for (int64_t b0 = 0; b0 < nc; b0 += kColBatch) {
        const int64_t bc = std::min<int64_t>(kColBatch, nc - b0);
        const ColDotsPlan pl = col_dots_plan(bc, h->nvec, h->sz.cus, 2);
        CHK(need_partials(h, pl.doubles));
        dim3 grid(pl.chunks, (unsigned)pl.groups);
        CHK(dispatch(h, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            hipLaunchKernelGGL(k_col_dots<T>, grid, dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld,
                               h->nvec, use_w ? (const T*)h->w : (const T*)nullptr, (const T*)rvec,
                               j0 + b0, (int)bc, d_cols, h->d_partials);
            return CDH_OK;
        }));
        hipLaunchKernelGGL(k_col_dots_reduce, dim3((unsigned)bc), dim3(64), 0, h->stream,
                           h->d_partials, pl.chunks, h->d_colout + 2 * b0);
        HIPCHK(h, hipGetLastError());
    }
    CHK(allreduce(h, h->d_colout, (size_t)(2 * nc)));
    return CDH_OK;
}

// ---- column loadings at the current residual: d_colout[j] = sum_i (x_ij r_i)^2 for all p columns (all shards) ----
// col_dots's batches and row chunks; read-only on the handle apart from bringing r up to date.
int32_t col_loadings(cdh_handle h) {
    CHK(sync_r(h));
    for (int64_t b0 = 0; b0 < h->p; b0 += kColBatch) {
        const int64_t bc = std::min<int64_t>(kColBatch, h->p - b0);
        const ColDotsPlan pl = col_dots_plan(bc, h->nvec, h->sz.cus, 1);
        CHK(need_partials(h, pl.doubles));
        dim3 grid(pl.chunks, (unsigned)pl.groups);
        CHK(dispatch(h, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            hipLaunchKernelGGL(k_col_loadings<T>, grid, dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld,
                               h->nvec, (const T*)h->r, b0, (int)bc, h->d_partials);
            return CDH_OK;
        }));
        hipLaunchKernelGGL(k_col_loadings_reduce, dim3((unsigned)bc), dim3(64), 0, h->stream,
                           h->d_partials, pl.chunks, h->d_colout + b0);
        HIPCHK(h, hipGetLastError());
    }
    CHK(allreduce(h, h->d_colout, (size_t)h->p));
    return CDH_OK;
}

// -> d_red[0..2] as ResidSums names them (v = r unless given; minus shift)
int32_t resid_moments_dev(cdh_handle h, const void* vec = nullptr, double shift = 0.0, bool sum_w = false) {
    if (!vec) { CHK(sync_r(h)); vec = h->r; }
    const int grid = elementwise_grid(h->nvec, kMomentsGridCap);
    CHK(dispatch(h, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, h->stream, h->nvec,
                               (const T*)vec, h->has_w ? (const T*)h->w : (const T*)nullptr, h->d_partials, shift, h->n);
        };
        if (sum_w) go(k_resid_moments<T, true>); else go(k_resid_moments<T>);
        return CDH_OK;
    }));
    hipLaunchKernelGGL(k_sum_records, dim3(1), dim3(kBlock), 0, h->stream, h->d_partials, grid, h->d_red);
    HIPCHK(h, hipGetLastError());
    CHK(allreduce(h, h->d_red, 4));
    return CDH_OK;
}

// ---- reading back what col_dots and resid_moments_dev left --------------------------------------------------------------------
// The pairs of nc columns, as col_dots lays them out in d_colout: (x.r, x.x) per column, weighted where the call was.
struct ColPairs {
    const double* v;
    ColPairs(const std::vector<double>& cd) : v(cd.data()) {}
    explicit ColPairs(const double* pairs) : v(pairs) {}
    double dot(int64_t j) const { return v[2 * j]; }
    double sq(int64_t j) const { return v[2 * j + 1]; }
};
// queue the copy of nc pairs into cd (resized to hold them); read_col_pairs waits for it as well
int32_t queue_col_pairs(cdh_handle h, int64_t nc, std::vector<double>& cd) {
    cd.resize((size_t)(2 * nc));
    HIPCHK(h, hipMemcpyAsync(cd.data(), h->d_colout, sizeof(double) * 2 * (size_t)nc, hipMemcpyDeviceToHost, h->stream));
    return CDH_OK;
}
int32_t read_col_pairs(cdh_handle h, int64_t nc, std::vector<double>& cd) {
    CHK(queue_col_pairs(h, nc, cd));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// The sums of resid_moments_dev over v (r, or the vector it was given, minus its shift), all shards.
struct ResidSums {
    double sum;     // sum v; with sum_w: sum w
    double sumsq;   // sum v^2
    double wsumsq;  // sum w v^2 (weights set)
};
// queue the copy into the pinned staging block; resid_sums(h) reads it once the stream has been waited for
int32_t queue_resid_sums(cdh_handle h) {
    HIPCHK(h, hipMemcpyAsync(h->h_red, h->d_red, sizeof(double) * 4, hipMemcpyDeviceToHost, h->stream));
    return CDH_OK;
}
inline ResidSums resid_sums(const cdh_handle_s* h) { return ResidSums{h->h_red[0], h->h_red[1], h->h_red[2]}; }
int32_t read_resid_sums(cdh_handle h, ResidSums* out) {
    CHK(queue_resid_sums(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *out = resid_sums(h);
    return CDH_OK;
}

// a 1-based coordinate, or a list of 1-based columns, lies inside the design
inline int32_t check_coordinate(cdh_handle h, int64_t k1) {
    return k1 < 1 || k1 > h->p ? fail(h, CDH_BAD_ARG, "coordinate out of range") : (int32_t)CDH_OK;
}
int32_t check_columns(cdh_handle h, const int64_t* idx1, int64_t m) {
    for (int64_t i = 0; i < m; ++i)
        if (idx1[i] < 1 || idx1[i] > h->p) return fail(h, CDH_BAD_ARG, "coordinate out of range");
    return CDH_OK;
}
