// cox_efron_host.hpp -- the chain of a handle set to Efron ties (cdh_glm_set_cox_ties), up to the partials; glm_launch<GlmCox>
// (cox_kernels.hpp) reduces and reads them back.  The mathematics and the chain are described at the top of cox_efron.hip, the
// Efron pair of buffers is cox_plan.hpp's (cox_efron_layout).  Host code only: it launches instantiations the other chains
// already have -- k_cox_exp<true>, k_cox_offsets<., true>, k_cox_scan<1, true, true>, k_cox_scan<2, false, true>, the tie
// groups' bounds where the strata's stand -- and calls cox_efron.hip for the three kernels of its own, which live in the
// library's second code object.  Included LAST by cdhip.hip, after cox_interval.hpp, so that no template is first used
// earlier than it was: the code object compiled from cdhip.hip stays what it was, byte for byte.
int32_t cox_launch_efron(cdh_handle h, int32_t k, bool apply, const GlmParams& pm) {
    const CoxPlan pl = cox_plan(h->ld, h->knobs.cox_grid);
    const CoxLayout lay = cox_layout(h->ld);
    const CoxEfronLayout el = cox_efron_layout(h->ld);
    double *d = h->glm.cox.d, *ed = h->glm.cox.ed;
    const int32_t *ii = h->glm.cox.i, *si = h->glm.cox.si;
    int32_t* ei = h->glm.cox.ei;
    const int32_t *first = ii + lay.first, *last = ii + lay.last, *sfirst = si + lay.sfirst, *slast = si + lay.slast;
    double *eT = d + lay.eT, *hA = d + lay.hA, *sums = d + lay.sums, *sums_h = d + lay.sums + kCoxMaxGrid;
    int32_t *heads = (int32_t*)h->glm.cox.si + lay.heads, *heads_h = heads + kCoxMaxGrid;
    double* esums = ed + el.sums;
    const double* weight = (const double*)h->glm.cox.sd + lay.weight;
    const double* off = h->glm.has_offset ? (const double*)h->glm.offset : (const double*)nullptr;
    const uint8_t* fold = k >= 0 ? (const uint8_t*)h->cv.fold : (const uint8_t*)nullptr;
    const CoxEfronBufs b{ii + lay.order, first, last, sfirst, eT, hA, d + lay.hB, sums_h, heads_h,
                         ed + el.cnt, ed + el.Sdv, ed + el.hc, ed + el.lg, ed + el.mm, esums, ei + el.heads_p, ei + el.heads_s};
    const CoxEfronRows rows{h->glm.labels, (double*)h->y, (double*)h->r, (double*)h->w, off, fold, (int)k, h->n, h->ld,
                            pm.wmin, pm.eta_max, weight, (double*)h->d_partials};
    static_assert(cox_efron_layout(32).Dv - cox_efron_layout(32).cnt == 32 && cox_efron_layout(32).hc2 - cox_efron_layout(32).hc == 32,
                  "k_cox_scan<2, ., .> takes its second vector ld doubles behind the first");
    const dim3 grid((unsigned)pl.grid), one(1), two(2), block(kCoxBlock);
    hipLaunchKernelGGL(k_cox_exp<true>, grid, block, 0, h->stream, b.order, rows.status, (const double*)rows.y, (const double*)rows.r,
                       off, fold, (int)k, h->n, h->ld, pl.tiles, pm.eta_max, eT, hA, sums, weight, slast, heads);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, cox_efron_mark(h->stream, pl, h->ld, b));
    hipLaunchKernelGGL((k_cox_offsets<true, true>), one, block, 0, h->stream, sums, (int)pl.grid, (const int32_t*)heads);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_offsets<false, true>), two, block, 0, h->stream, esums, (int)pl.grid, (const int32_t*)b.heads_p);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_offsets<true, true>), one, block, 0, h->stream, esums + 2 * kCoxMaxGrid, (int)pl.grid,
                       (const int32_t*)b.heads_s);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_scan<1, true, true>), grid, block, 0, h->stream, eT, (const double*)sums, h->ld, pl.tiles, slast);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_scan<2, false, true>), grid, block, 0, h->stream, b.cnt, (const double*)esums, h->ld, pl.tiles, first);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_scan<1, true, true>), grid, block, 0, h->stream, b.Sdv, (const double*)(esums + 2 * kCoxMaxGrid), h->ld,
                       pl.tiles, last);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, cox_efron_hazard(h->stream, pl, h->ld, b));
    hipLaunchKernelGGL((k_cox_offsets<false, true>), two, block, 0, h->stream, sums_h, (int)pl.grid, (const int32_t*)heads_h);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_offsets<false, true>), two, block, 0, h->stream, esums + 3 * kCoxMaxGrid, (int)pl.grid,
                       (const int32_t*)b.heads_p);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_scan<2, false, true>), grid, block, 0, h->stream, hA, (const double*)sums_h, h->ld, pl.tiles, sfirst);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL((k_cox_scan<2, false, true>), grid, block, 0, h->stream, b.hc, (const double*)(esums + 3 * kCoxMaxGrid), h->ld,
                       pl.tiles, first);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, cox_efron_apply(h->stream, pl, b, rows, apply));
    return CDH_OK;
}
