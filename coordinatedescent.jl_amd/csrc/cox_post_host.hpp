// cox_post_host.hpp -- the bodies of cdh_glm_cox_residuals and cdh_glm_cox_baseline: the refusals, the post group's scratch
// (cox_plan.hpp: cox_post_layout), the handle's own read-only step and the calls into cox_post.hip, whose kernels live in the
// library's third code object.  Host code only, included by cdhip.hip inside its anonymous namespace after cox_kernels.hpp: it
// launches no kernel itself, so the code object compiled from cdhip.hip stays what it was, byte for byte.
//
// Both exports evaluate the model at the iterate the handle holds, with no row held out (the fold ids are not read), and leave
// y, w, r and beta as they are: the step is the one cdh_glm_cox_irls(k = -1, apply = 0) runs, catch-up of r included, and the
// post kernels only read what it left in the Cox group's scratch.

// what both exports refuse of the handle and of eta_max, before anything is touched
int32_t cox_post_refuse(cdh_handle h, double eta_max) {
    CHK(glm_refuse(h));
    if (!h->glm.set || h->glm.family != GlmData::Cox)
        return fail(h, CDH_BAD_ARG, "no survival data are set: call cdh_glm_set_survival first");
    if (!(eta_max > 0.0 && eta_max <= 700.0)) return fail(h, CDH_BAD_ARG, "need 0 < eta_max <= 700");
    return CDH_OK;
}

// The post group, allocated whole by the first call that needs it and before anything else happens; then the read-only step.
// Its record is not used and neither is its wmin (A, T and the scans do not depend on it).  in, b: what cox_post.hip takes.
int32_t cox_post_step(cdh_handle h, double eta_max, CoxPostIn& in, CoxPostBufs& b) {
    const GlmParams pm{1e-5, eta_max};
    double out5[kCoxVals];
    CHK(glm_check<GlmCox>(h, -1, 0, pm, out5));
    HIPCHK(h, hipSetDevice(h->device));
    const CoxPostLayout pl = cox_post_layout(h->ld);
    if (!h->glm.cox.pd) {
        DevBuf<double> fresh_pd;
        DevBuf<int32_t> fresh_pi;
        HIPCHK(h, fresh_pd.alloc((size_t)pl.doubles * sizeof(double)));
        HIPCHK(h, fresh_pi.alloc((size_t)pl.ints * sizeof(int32_t)));
        HIPCHK(h, hipMemsetAsync(fresh_pd, 0, (size_t)pl.doubles * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(fresh_pi, 0, (size_t)pl.ints * sizeof(int32_t), h->stream));
        h->glm.cox.pd = std::move(fresh_pd);
        h->glm.cox.pi = std::move(fresh_pi);
    }
    CHK(glm_catch_up(h));
    CHK(glm_launch<GlmCox>(h, -1, false, pm, out5));
    const CoxLayout lay = cox_layout(h->ld);
    const CoxState& cx = h->glm.cox;
    const double* d = cx.d;
    const int32_t* ii = cx.i;
    const int32_t* si = cx.strata ? (const int32_t*)cx.si : (const int32_t*)nullptr;
    const int32_t* vi = cx.interval ? (const int32_t*)cx.vi : (const int32_t*)nullptr;
    in = CoxPostIn{ii + lay.order, ii + lay.first, ii + lay.last,
                   si ? si + lay.sfirst : nullptr, vi ? vi + lay.lo : nullptr, vi ? vi + lay.enter : nullptr,
                   d + lay.eT, cx.interval ? (const double*)cx.vd + lay.T2 : nullptr, d + lay.hA, d + lay.hB,
                   cx.efron ? (const double*)cx.ed + cox_efron_layout(h->ld).hc : nullptr,
                   (const double*)h->glm.labels, (const double*)h->y, (const double*)h->r,
                   h->glm.has_offset ? (const double*)h->glm.offset : (const double*)nullptr,
                   cx.strata ? (const double*)cx.sd + lay.weight : nullptr, d + lay.time,
                   si ? si + lay.strata : nullptr, h->n, h->ld, eta_max};
    double* pd = h->glm.cox.pd;
    int32_t* pi = h->glm.cox.pi;
    b = CoxPostBufs{pd + pl.dv, pd + pl.flag, pd + pl.out, pd + pl.sums, pd + pl.total, pi + pl.stratum, pi + pl.slotpos, pi + pl.heads};
    return CDH_OK;
}

int32_t cox_post_residuals(cdh_handle h, double eta_max, void* host_cumhaz, void* host_martingale, void* host_deviance) {
    CHK(cox_post_refuse(h, eta_max));
    if (!host_cumhaz && !host_martingale && !host_deviance)
        return fail(h, CDH_BAD_ARG, "host_cumhaz, host_martingale and host_deviance are all NULL");
    CoxPostIn in;
    CoxPostBufs b;
    CHK(cox_post_step(h, eta_max, in, b));
    void* const host[3] = {host_cumhaz, host_martingale, host_deviance};
    const bool want[3] = {host[0] != nullptr, host[1] != nullptr, host[2] != nullptr};
    const CoxPostChain chain = h->glm.cox.efron ? CoxPostChain::Efron
                               : h->glm.cox.interval ? CoxPostChain::Interval : CoxPostChain::Censored;
    const CoxPlan plan = cox_plan(h->ld, h->knobs.cox_grid);
    HIPCHK(h, cox_post_table(h->stream, plan, in, b));          // the rows read hA where the table reads it; out is theirs afterwards
    HIPCHK(h, cox_post_rows(h->stream, plan, chain, in, b, want));
    for (int i = 0; i < 3; ++i)
        if (want[i])
            HIPCHK(h, hipMemcpyAsync(host[i], b.out + (int64_t)i * h->ld, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost,
                                     h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

int32_t cox_post_baseline(cdh_handle h, double eta_max, int64_t capacity, int32_t* host_stratum, void* host_time,
                          void* host_n_event, void* host_risk_sum, void* host_cumhaz, void* host_cumvar, int64_t* count) {
    CHK(cox_post_refuse(h, eta_max));
    NEED_P(h, count);
    if (capacity < 0) return fail(h, CDH_BAD_ARG, "capacity is negative");
    CoxPostIn in;
    CoxPostBufs b;
    CHK(cox_post_step(h, eta_max, in, b));
    HIPCHK(h, cox_post_table(h->stream, cox_plan(h->ld, h->knobs.cox_grid), in, b));
    double total = 0.0;
    HIPCHK(h, hipMemcpyAsync(&total, b.total, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int64_t m = (int64_t)total;
    *count = m;
    if (m > capacity) {
        char buf[160];
        snprintf(buf, sizeof buf, "the baseline table has %lld rows and capacity is %lld", (long long)m, (long long)capacity);
        return fail(h, CDH_BAD_ARG, buf);
    }
    void* const host[kCoxPostCols] = {host_time, host_n_event, host_risk_sum, host_cumhaz, host_cumvar};
    if (host_stratum)
        HIPCHK(h, hipMemcpyAsync(host_stratum, b.stratum, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    for (int c = 0; c < kCoxPostCols; ++c)
        if (host[c])
            HIPCHK(h, hipMemcpyAsync(host[c], b.out + (int64_t)c * h->ld, (size_t)m * sizeof(double), hipMemcpyDeviceToHost,
                                     h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}
