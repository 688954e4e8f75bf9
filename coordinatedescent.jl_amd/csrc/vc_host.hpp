// vc_host.hpp -- the host side of varying-coefficient mode (varying_coefficient_lasso.jl:30-79): the body of cdh_vc_set_data, a
// point of the design (vc_point: weights, expansion, weighted column scales; its batches are stats_plan.hpp's to say), and the
// scratch, the launch body and the group planners of cdh_vc_gram and cdh_vc_gram_batch (vc_gram.hpp).  Included by cdhip.hip, in
// its anonymous namespace, where this code has always stood (behind the GLM exports, ahead of cdh_get_X_row's body: the place
// decides the order of the kernels in the code object).

int32_t vc_refuse_shards(cdh_handle h) {
    if (h->n != h->n_total || h->xs.sharded())
        return fail(h, CDH_BAD_ARG, "varying-coefficient mode does not run on row-sharded handles");
    return CDH_OK;
}

int32_t vc_set_data(cdh_handle h, int64_t p_base, int32_t degree, const void* host_X, int64_t ld, const void* host_z) {
    NEED_P(h, host_X);
    NEED_P(h, host_z);
    if (degree < 0 || degree > 3) return fail(h, CDH_BAD_ARG, "the polynomial degree must be 0 .. 3");
    CHK(vc_refuse_shards(h));
    if (h->loss != CDH_WLS || p_base < 1 || h->p != p_base * (degree + 1) || ld < h->n)
        return fail(h, CDH_DIM_MISMATCH, "need a CDH_WLS handle with p == p_base * (degree + 1) and ld >= n");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t colbytes = (size_t)h->ld * h->esz;
    DevBuf<void> z;                      // complete before the handle changes: a failed allocation leaves it as it was
    if (!h->vc_z) {
        HIPCHK(h, z.alloc(colbytes));
        HIPCHK(h, hipMemsetAsync(z, 0, colbytes, h->stream));
    }
    CHK(design_changes(h, true));
    if (!h->vc_z) h->vc_z = std::move(z);
    h->vc_pbase = p_base; h->vc_degree = degree;
    // base column j -> column j (degree + 1): one strided copy
    HIPCHK(h, hipMemcpy2DAsync(h->X, colbytes * (size_t)(degree + 1), host_X, (size_t)ld * h->esz, (size_t)h->n * h->esz,
                               (size_t)p_base, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->vc_z, host_z, (size_t)h->n * h->esz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// One point of the varying-coefficient design: weights, expansion, weighted column scales -- around z0 (row0 < 0), or around
// the stored z[row0] with that row's weight zero and the screening scores |X_j'Wy| on top (the leave-one-out point).
int32_t vc_point(cdh_handle h, int32_t kernel_kind, double bandwidth, double z0, int64_t row0, double* out_std,
                 double* out_scores) {
    const bool loo = row0 >= 0;
    if (h->vc_degree < 0) return fail(h, CDH_BAD_ARG, "a varying-coefficient point needs cdh_vc_set_data first");
    if (kernel_kind != kVcGaussian && kernel_kind != kVcEpanechnikov) return fail(h, CDH_BAD_ARG, "unknown smoothing kernel");
    if (!(bandwidth > 0.0) || !std::isfinite(bandwidth)) return fail(h, CDH_BAD_ARG, "the bandwidth must be positive");
    if (!std::isfinite(z0)) return fail(h, CDH_BAD_ARG, "z0 must be finite");
    CHK(vc_refuse_shards(h));
    if (h->loss != CDH_WLS) return fail(h, CDH_BAD_ARG, "varying-coefficient mode needs the CDH_WLS loss");
    HIPCHK(h, hipSetDevice(h->device));
    CHK(design_changes(h, true));
    CHK(ensure_weights_buffer(h));
    const int Q = h->vc_degree, Q1 = Q + 1;
    HIPCHK(h, h->prof.begin(h->stream));
    const int wgrid = elementwise_grid(h->nvec, kWeightsGridCap);
    CHK(dispatch(h, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        hipLaunchKernelGGL(k_vc_weights<T>, dim3(wgrid), dim3(kBlock), 0, h->stream, (const T*)h->vc_z, (T*)h->w, h->n,
                           h->nvec, (int)kernel_kind, bandwidth, z0, row0);
        return CDH_OK;
    }));
    HIPCHK(h, hipGetLastError());
    h->has_w = true;
    // What comes back.  Degree 0 expands nothing: the weighted scales of the base columns and their dots with y are col_dots'
    // pairs.  Otherwise d_colout holds the p sums of w v^2 and, with a left-out row, the p sums of w v y behind them.
    std::vector<double> cd;
    if (Q == 0) {
        CHK(col_dots(h, 0, h->p, h->y, true));
        CHK(queue_col_pairs(h, h->p, cd));
        HIPCHK(h, h->prof.stop(h->stream));   // (the bracket closes in stream order before the wait: one stop per branch, one end below)
    } else {
        for (int64_t b = 0; b < vc_batches(h->p); ++b) {
            const VcBatch B = vc_batch(h->p, Q, h->nvec, h->sz.cus, loo, b);
            const unsigned bases = (unsigned)(B.jb1 - B.jb0);
            CHK(need_partials(h, B.partials));
            CHK(dispatch(h, [&](auto* t) {
                using T = std::remove_pointer_t<decltype(t)>;
                auto go = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, dim3((unsigned)B.chunks, bases), dim3(kBlock), 0, h->stream,
                                       (T*)h->X, h->ld, h->nvec, (const T*)h->vc_z, (const T*)h->w, (T)z0, B.jb0, h->d_partials,
                                       (const T*)h->y, row0);
                };
                auto by_degree = [&](auto left_out) {
                    constexpr bool kLoo = decltype(left_out)::value;
                    if (Q == 1) go(k_vc_expand<T, 1, kLoo>); else if (Q == 2) go(k_vc_expand<T, 2, kLoo>); else go(k_vc_expand<T, 3, kLoo>);
                };
                if (loo) by_degree(std::true_type{}); else by_degree(std::false_type{});
                return CDH_OK;
            }));
            hipLaunchKernelGGL(k_vc_reduce, dim3(bases * (unsigned)Q1), dim3(64), 0, h->stream, h->d_partials, B.chunks,
                               B.jb0 * Q1, B.b0, B.b1, h->d_colout);
            if (loo)
                hipLaunchKernelGGL(k_vc_reduce, dim3(bases * (unsigned)Q1), dim3(64), 0, h->stream, h->d_partials + B.table,
                                   B.chunks, B.jb0 * Q1, B.b0, B.b1, h->d_colout + h->p);
            HIPCHK(h, hipGetLastError());
        }
        HIPCHK(h, h->prof.stop(h->stream));
        cd.resize((size_t)(loo ? 2 * h->p : h->p));
        HIPCHK(h, hipMemcpyAsync(cd.data(), h->d_colout, sizeof(double) * cd.size(), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, h->prof.end(vc_point_launches(h->p, Q), vc_point_bytes(h->n, h->esz, h->p)));
    const ColPairs pairs(cd);
    if (out_std) for (int64_t j = 0; j < h->p; ++j) out_std[j] = std::sqrt((Q == 0 ? pairs.sq(j) : cd[(size_t)j]) / (double)h->n_total);
    if (out_scores) for (int64_t j = 0; j < h->p; ++j) out_scores[j] = std::fabs(Q == 0 ? pairs.dot(j) : cd[(size_t)(h->p + j)]);
    return CDH_OK;
}

// The weighted Gram matrix and right-hand side of the expanded design around one point, straight from the base design
// (_expand_Xt_w_X!, _expand_Xt_w_Y!: varying_coefficient_lasso.jl:572-647): one pass over the listed base columns, z and y.
// Reads the handle's data and writes only its own scratch: residual, cache, weights, expanded columns and iterate stay.
// A batch of points per launch (the loops of locpoly on a grid, lvocv_locpoly and split_locpoly,
// varying_coefficient_lasso.jl:217-235, 348-380, 383-409, over :572-647) is the same body over more points: point t of
// cdh_vc_gram_batch is cdh_vc_gram at (bandwidth[t], z0[t], leave_out_row0[t]), bit for bit.
static_assert(kVgbMaxPoints == CDH_VC_GRAM_MAX_POINTS && kVgMaxCols == CDH_VC_GRAM_MAX_COLS, "cdhip.h names the limits the headers derive");
int32_t vc_gram_scratch(cdh_handle h) {
    VcGramScratch& g = h->vg;
    if (g.ready) return CDH_OK;
    VcGramScratch s;                     // complete before the handle changes
    const size_t nrec = (size_t)vc_gram_rec(kVgMaxDegree, kVgMaxCols).n;
    HIPCHK(h, s.partials.alloc(sizeof(double) * (size_t)kVgPartialDoubles));
    HIPCHK(h, s.out.alloc(sizeof(double) * nrec));
    HIPCHK(h, s.in.alloc(sizeof(VcGramInput)));
    HIPCHK(h, s.e.alloc((size_t)h->ld * h->esz));
    HIPCHK(h, s.h_out.alloc(sizeof(double) * nrec));
    HIPCHK(h, s.h_in.alloc(sizeof(VcGramInput)));
    s.ready = true;
    g = std::move(s);
    return CDH_OK;
}
int32_t vc_gram_batch_scratch(cdh_handle h) {
    VcGramBatchScratch& g = h->vgb;
    if (g.ready) return CDH_OK;
    VcGramBatchScratch s;                // complete before the handle changes
    HIPCHK(h, s.partials.alloc(sizeof(double) * (size_t)kVgbPartialDoubles));
    HIPCHK(h, s.out.alloc(sizeof(double) * (size_t)kVgbOutDoubles));
    HIPCHK(h, s.pts.alloc(sizeof(VcGramPoint) * (size_t)kVgbMaxGroupPoints));
    HIPCHK(h, s.h_out.alloc(sizeof(double) * (size_t)kVgbOutDoubles));
    HIPCHK(h, s.h_pts.alloc(sizeof(VcGramPoint) * (size_t)kVgbMaxGroupPoints));
    s.ready = true;
    g = std::move(s);
    return CDH_OK;
}

// The body of both exports, after their checks and their scratch: the points t < m in `ngroups` launch groups, each laid out
// by group(h, m, mb, grp, &L) (CDH_OK, or the export's refusal), in the buffers b and the regime the export names.  Per call
// the columns and e go to the device once; per group the points, k_vc_moments, k_vc_moments_reduce, one copy back, one
// synchronise.  Where b's point is the one behind the columns (cdh_vc_gram), one copy takes columns and point `together`.
struct VcGramGroup { int64_t first, pts, per, gy; };   // points first .. first + pts - 1 on a grid (G, gy), `per` a share (resident)
typedef int32_t (*VcGramPlan)(cdh_handle h, int64_t m, int64_t mb, int64_t grp, VcGramGroup* L);
int32_t vc_gram_run(cdh_handle h, int32_t kernel_kind, int64_t m, const double* bandwidth, const double* z0,
                    const int64_t* leave_out_row0, int32_t wpow, const void* host_e, int64_t mb, const int64_t* base_idx1,
                    double* out_G, double* out_c, double* out_sum_w, const VcGramBufs& b, bool resident, int64_t ngroups,
                    VcGramPlan group) {
    VcGramScratch& g = h->vg;
    VcGramInput* const d_in = g.in;
    const int Q = h->vc_degree;
    const int64_t n = h->n, Q1 = Q + 1, ep = mb * Q1;
    const VcGramRec R = vc_gram_rec(Q, mb);
    const int G = vc_gram_grid(n, Q, mb);
    const bool together = b.h_pts == &g.h_in->pt;
    for (int64_t i = 0; i < mb; ++i) g.h_in->cols[i] = (base_idx1[i] - 1) * Q1;      // base column j sits at column j (Q + 1)
    if (!together)
        HIPCHK(h, hipMemcpyAsync(d_in->cols, g.h_in->cols, sizeof(int64_t) * (size_t)mb, hipMemcpyHostToDevice, h->stream));
    if (host_e) HIPCHK(h, hipMemcpyAsync(g.e, host_e, (size_t)n * h->esz, hipMemcpyHostToDevice, h->stream));   // once per call
    for (int64_t grp = 0; grp < ngroups; ++grp) {
        VcGramGroup L;
        CHK(group(h, m, mb, grp, &L));
        for (int64_t t = 0; t < L.pts; ++t) {
            const int64_t lo = leave_out_row0 ? leave_out_row0[L.first + t] : -1;
            b.h_pts[t] = VcGramPoint{lo >= 0 ? 0.0 : z0[L.first + t], bandwidth[L.first + t], lo};
        }
        if (together) HIPCHK(h, hipMemcpyAsync(d_in, g.h_in, sizeof(VcGramInput), hipMemcpyHostToDevice, h->stream));
        else HIPCHK(h, hipMemcpyAsync(b.pts, b.h_pts, sizeof(VcGramPoint) * (size_t)L.pts, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, h->prof.begin(h->stream));
        CHK(dispatch(h, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            auto go = [&](auto streamed, auto res) {
                hipLaunchKernelGGL(resident ? res : streamed, dim3((unsigned)G, (unsigned)L.gy), dim3(kVgThreads), 0, h->stream,
                                   (const T*)h->X, h->ld, n, (const T*)h->vc_z, out_c ? (const T*)h->y : (const T*)nullptr,
                                   host_e ? (const T*)g.e : (const T*)nullptr, (const int64_t*)d_in->cols, (int)mb, (int)kernel_kind,
                                   (int)wpow, (const VcGramPoint*)b.pts, (int)L.pts, (int)L.per, b.partials);
            };
            if (Q == 0) go(k_vc_moments<T, 0, false>, k_vc_moments<T, 0, true>);
            else if (Q == 1) go(k_vc_moments<T, 1, false>, k_vc_moments<T, 1, true>);
            else if (Q == 2) go(k_vc_moments<T, 2, false>, k_vc_moments<T, 2, true>);
            else go(k_vc_moments<T, 3, false>, k_vc_moments<T, 3, true>);
            return CDH_OK;
        }));
        hipLaunchKernelGGL(k_vc_moments_reduce, dim3((unsigned)((R.n + kVgThreads - 1) / kVgThreads), (unsigned)L.pts), dim3(kVgThreads),
                           0, h->stream, (const double*)b.partials, G, R.n, b.out);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, h->prof.stop(h->stream));
        HIPCHK(h, hipMemcpyAsync(b.h_out, b.out, sizeof(double) * (size_t)(L.pts * R.n), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, h->prof.end(2, 0.0));  // cdh_profile_begin/end: the device time of the two launches
        for (int64_t t = 0; t < L.pts; ++t) {
            const double* rec = b.h_out + t * R.n;
            vc_gram_scatter(Q, mb, rec, out_G + (L.first + t) * ep * ep, out_c ? out_c + (L.first + t) * ep : nullptr);
            if (out_sum_w) out_sum_w[L.first + t] = rec[R.off_w];
        }
    }
    return CDH_OK;
}

// One point: a batch of one in the small tier, always in the streamed regime (vc_gram_batch_types.hpp: vgb_resident)
int32_t vc_gram_one_group(cdh_handle, int64_t, int64_t, int64_t, VcGramGroup* L) {
    *L = VcGramGroup{0, 1, 1, 1};
    return CDH_OK;
}
// Many points: the plan of the call is vc_gram_batch_types.hpp's
int32_t vc_gram_batch_group(cdh_handle h, int64_t m, int64_t mb, int64_t grp, VcGramGroup* L) {
    const int Q = h->vc_degree;
    const int64_t n = h->n, pts = vgb_group_size(n, Q, mb, m, grp), gy = vgb_grid_y(n, Q, mb, pts);
    *L = VcGramGroup{vgb_group_first(n, Q, mb, grp), pts, vgb_share_points(n, Q, mb, pts), gy};
    if (pts < 1 || vgb_rec_offset(n, Q, mb, pts, 0) > kVgbPartialDoubles || pts * vc_gram_rec(Q, mb).n > kVgbOutDoubles ||
        pts > kVgbMaxGroupPoints || gy < 1 || gy > 65535 || vgb_share_begin(n, Q, mb, pts, gy) != pts)
        return fail(h, CDH_BAD_ARG, "cdh_vc_gram_batch: the plan of this call does not fit its scratch");
    return CDH_OK;
}
