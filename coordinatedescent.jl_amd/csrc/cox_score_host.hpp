// cox_score_host.hpp -- the body of cdh_glm_cox_score: the refusals, the score group's scratch (cox_plan.hpp: cox_score_layout,
// cox_score_grow), the handle's own read-only step and the calls into cox_score.hip, whose kernels live in the library's fifth
// code object.  Host code only, included by cdhip.hip inside its anonymous namespace after cox_concordance_host.hpp: it
// launches no kernel itself, so the code object compiled from cdhip.hip stays what it was, byte for byte.
//
// The call evaluates the model at the iterate the handle holds, with no row held out (the fold ids are not read), and leaves
// y, w, r and beta as they are: the step is the one cdh_glm_cox_irls(k = -1, apply = 0) runs, catch-up of r included, and the
// score kernels only read what it left in the Cox group's scratch, the handle's vectors and the design.

// The score group for at least m columns: allocated whole by the first call, regrown whole when a later call asks for more
// columns than it holds, and the handle keeps the old one until the new one is complete.
int32_t cox_score_scratch(cdh_handle h, int64_t m) {
    CoxState& cx = h->glm.cox;
    if (cx.qd && cx.score_cols >= m) return CDH_OK;
    const int64_t cols = cox_score_grow(cx.qd ? cx.score_cols : 0, m);
    const CoxScoreLayout sl = cox_score_layout(h->ld, cols);
    DevBuf<double> fresh_d;
    DevBuf<int32_t> fresh_i;
    HIPCHK(h, fresh_d.alloc((size_t)sl.doubles * sizeof(double)));
    HIPCHK(h, fresh_i.alloc((size_t)sl.ints * sizeof(int32_t)));
    HIPCHK(h, hipMemsetAsync(fresh_d, 0, (size_t)sl.doubles * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(fresh_i, 0, (size_t)sl.ints * sizeof(int32_t), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (nothing in flight reads the old group when it goes)
    cx.qd = std::move(fresh_d);
    cx.qi = std::move(fresh_i);
    cx.score_cols = cols;
    return CDH_OK;
}

int32_t cox_score(cdh_handle h, double eta_max, int64_t m, const int64_t* idx1, const double* host_centre, double* host_centre_out,
                  void* host_schoenfeld, void* host_score, double* host_info) {
    CHK(cox_post_refuse(h, eta_max));
    if (m < 1 || m > kCoxScoreMaxCols) return fail(h, CDH_BAD_ARG, "cdh_glm_cox_score: need 1 <= m <= 64 columns");
    NEED_P(h, idx1);
    CHK(check_columns(h, idx1, m));
    if (!host_schoenfeld && !host_score && !host_info)
        return fail(h, CDH_BAD_ARG, "host_schoenfeld, host_score and host_info are all NULL");
    if (host_centre)
        for (int64_t c = 0; c < m; ++c)
            if (!(fabs(host_centre[c]) <= 1.7976931348623157e308)) {          // (a NaN fails the comparison)
                char buf[96];
                snprintf(buf, sizeof buf, "host_centre[%lld] = %g is not finite", (long long)c, host_centre[c]);
                return fail(h, CDH_BAD_ARG, buf);
            }
    if (h->glm.cox.interval) return fail(h, CDH_BAD_ARG, "cdh_glm_cox_score is not offered with start-stop times yet");
    if (h->glm.cox.efron) return fail(h, CDH_BAD_ARG, "cdh_glm_cox_score is not offered with Efron ties yet");
    const GlmParams pm{1e-5, eta_max};
    double out5[kCoxVals];
    CHK(glm_check<GlmCox>(h, -1, 0, pm, out5));
    HIPCHK(h, hipSetDevice(h->device));
    CHK(cox_score_scratch(h, m));
    CHK(glm_catch_up(h));
    CHK(glm_launch<GlmCox>(h, -1, false, pm, out5));
    const CoxLayout lay = cox_layout(h->ld);
    const CoxState& cx = h->glm.cox;
    const CoxScoreLayout sl = cox_score_layout(h->ld, cx.score_cols);
    const double* d = cx.d;
    const int32_t* ii = cx.i;
    const int32_t* si = cx.strata ? (const int32_t*)cx.si : (const int32_t*)nullptr;
    const CoxScoreIn in{ii + lay.order, ii + lay.first, ii + lay.last, si ? si + lay.sfirst : nullptr, si ? si + lay.slast : nullptr,
                        d + lay.eT, d + lay.hA, (const double*)h->glm.labels, (const double*)h->y, (const double*)h->r,
                        h->glm.has_offset ? (const double*)h->glm.offset : (const double*)nullptr,
                        cx.strata ? (const double*)cx.sd + lay.weight : (const double*)nullptr, (const double*)h->X,
                        h->n, h->ld, m, eta_max};
    double* q = cx.qd;
    int32_t* qi = cx.qi;
    const int64_t cols = cx.score_cols;
    const CoxScoreBufs b{q + sl.e, q + sl.ev, q + sl.h, q + sl.dvk, q + sl.wA, q + sl.xt, q + sl.N, q + sl.Q, q + sl.sums,
                         q + sl.sums + cols * kCoxMaxGrid, q + sl.mu, q + sl.out, q + sl.out + cols * h->ld, q + sl.part, q + sl.info,
                         qi + sl.heads, qi + sl.heads + kCoxMaxGrid, qi + sl.idx};
    int32_t idx0[kCoxScoreMaxCols];
    for (int64_t c = 0; c < m; ++c) idx0[c] = (int32_t)(idx1[c] - 1);
    // (the stream is idle: the step's launch ended in a synchronise.  Plain copies: idx0 is this frame's and the centres are the
    // caller's, and neither may be read after an early return)
    HIPCHK(h, hipMemcpy(b.idx, idx0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
    if (host_centre) HIPCHK(h, hipMemcpy(b.mu, host_centre, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
    else HIPCHK(h, cox_score_centres(h->stream, in, b));
    HIPCHK(h, cox_score_run(h->stream, cox_plan(h->ld, h->knobs.cox_grid), in, b, host_schoenfeld != nullptr, host_score != nullptr,
                            host_info != nullptr));
    const size_t rows = (size_t)h->n * (size_t)m * sizeof(double);
    if (host_centre_out) HIPCHK(h, hipMemcpyAsync(host_centre_out, b.mu, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (host_schoenfeld) HIPCHK(h, hipMemcpyAsync(host_schoenfeld, b.sch, rows, hipMemcpyDeviceToHost, h->stream));
    if (host_score) HIPCHK(h, hipMemcpyAsync(host_score, b.score, rows, hipMemcpyDeviceToHost, h->stream));
    if (host_info) HIPCHK(h, hipMemcpyAsync(host_info, b.info, (size_t)(m * m) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}
