// cox_concordance_host.hpp -- the body of cdh_glm_cox_concordance: the refusals, the concordance group's scratch and order
// (cox_plan.hpp: cox_conc_layout, cox_conc_order), the catch-up of r and the call into cox_concordance.hip, whose kernels live
// in the library's fourth code object.  Host code only, included by cdhip.hip inside its anonymous namespace after
// cox_post_host.hpp: it launches no kernel itself, so the code object compiled from cdhip.hip stays what it was.
//
// The call evaluates the model at the iterate the handle holds and leaves y, w, r, beta and the step's scratch as they are:
// it reads y, r, the offset, the weights and the fold ids, and writes only its own group.  The tie rule does not enter.

// The group, allocated whole by the first call after a setter of survival data (which drops it: cox_set_survival), and the
// order: the handle's order, tie groups, strata bounds and statuses come back from the device ONCE per data set, the
// concordance order and every event's range go up.  Nothing of the handle changes before all of it has succeeded.
int32_t cox_conc_prepare(cdh_handle h) {
    if (h->glm.cox.cd) return CDH_OK;
    const CoxLayout lay = cox_layout(h->ld);
    const CoxConcLayout cl = cox_conc_layout(h->ld);
    const CoxState& cx = h->glm.cox;
    const size_t idx = (size_t)h->ld * sizeof(int32_t);
    std::vector<int32_t> order((size_t)h->ld), last((size_t)h->ld), slast;
    std::vector<double> status((size_t)h->n);
    HIPCHK(h, hipMemcpyAsync(order.data(), (const int32_t*)cx.i + lay.order, idx, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(last.data(), (const int32_t*)cx.i + lay.last, idx, hipMemcpyDeviceToHost, h->stream));
    if (cx.strata) {
        slast.resize((size_t)h->ld);
        HIPCHK(h, hipMemcpyAsync(slast.data(), (const int32_t*)cx.si + lay.slast, idx, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(status.data(), (const double*)h->glm.labels, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> corder, qa, qb;
    cox_conc_order(h->n, h->ld, cl.N, order.data(), last.data(), cx.strata ? slast.data() : nullptr, status.data(), corder, qa, qb);
    DevBuf<double> fresh_d;
    DevBuf<int32_t> fresh_i;
    HIPCHK(h, fresh_d.alloc((size_t)cl.doubles * sizeof(double)));
    HIPCHK(h, fresh_i.alloc((size_t)cl.ints * sizeof(int32_t)));
    int32_t* ci = fresh_i;
    const size_t nb = (size_t)cl.N * sizeof(int32_t);
    HIPCHK(h, hipMemsetAsync(fresh_d, 0, (size_t)cl.doubles * sizeof(double), h->stream));
    HIPCHK(h, hipMemcpyAsync(ci + cl.order, corder.data(), nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(ci + cl.qa, qa.data(), nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(ci + cl.qb, qb.data(), nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (the host vectors are pageable: the copies are done here)
    h->glm.cox.cd = std::move(fresh_d);
    h->glm.cox.ci = std::move(fresh_i);
    return CDH_OK;
}

int32_t cox_concordance(cdh_handle h, int32_t k, double* out4) {
    CHK(glm_refuse(h));
    if (!h->glm.set || h->glm.family != GlmData::Cox)
        return fail(h, CDH_BAD_ARG, "no survival data are set: call cdh_glm_set_survival first");
    CHK(glm_refuse_k(h, k));
    if (!out4) return fail(h, CDH_BAD_ARG, "out4 is NULL");
    if (h->glm.cox.interval) return fail(h, CDH_BAD_ARG, "concordance with start-stop times is not offered yet");
    HIPCHK(h, hipSetDevice(h->device));
    CHK(cox_conc_prepare(h));
    CHK(glm_catch_up(h));
    const CoxState& cx = h->glm.cox;
    const CoxConcLayout cl = cox_conc_layout(h->ld);
    const CoxConcIn in{(const double*)h->y, (const double*)h->r,
                       h->glm.has_offset ? (const double*)h->glm.offset : (const double*)nullptr,
                       cx.strata ? (const double*)cx.sd + cox_layout(h->ld).weight : (const double*)nullptr,
                       k >= 0 ? (const uint8_t*)h->cv.fold : (const uint8_t*)nullptr, k, h->n};
    double* d = cx.cd;
    const int32_t* ci = cx.ci;
    const CoxConcBufs b{ci + cl.order, ci + cl.qa, ci + cl.qb, d + cl.key0, d + cl.v0, d + cl.ka, d + cl.pa, d + cl.kb,
                        d + cl.pb, d + cl.L, d + cl.E, d + cl.G, d + cl.part, d + cl.out, cl.N, cl.tiles};
    HIPCHK(h, cox_conc_run(h->stream, in, b));
    HIPCHK(h, hipMemcpyAsync(out4, b.out, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}
