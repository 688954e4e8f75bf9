// cox_score.hpp -- what the library's translation units share of cdh_glm_cox_score (score and Schoenfeld residuals and the
// information matrix of a fitted Cox model): the launch sequence that cox_score.hip defines and cdhip.hip calls
// (cox_score_host.hpp) AFTER the handle's own read-only step, over the scratch that step leaves and the resident design.
// Plain functions over the stream, raw device pointers and the plan of cox_plan.hpp: the handle stays cdhip.hip's.  Each returns
// the first error of its launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cox_plan.hpp"

// What the step left and what the handle holds.  sfirst, slast and weight are nullptr on a plain handle (one stratum, unit
// weights), offset without one.  X: the design, column-major, ld apart, fp64.
struct CoxScoreIn {
    const int32_t *order, *first, *last, *sfirst, *slast;
    const double *T, *hA;
    const double *status, *y, *r, *offset, *weight;
    const double* X;
    int64_t n, ld, m;
    double eta_max;
};

// the score group's scratch, by cox_score_layout(ld, cap): the per-column vectors are ld apart, the runs' sums kCoxMaxGrid
struct CoxScoreBufs {
    double *e, *ev, *h, *dvk, *wA, *xt, *N, *Q, *sums_N, *sums_Q, *mu, *sch, *score, *part, *info;
    int32_t *heads_N, *heads_Q, *idx;
};

// mu[c] becomes the mean of column idx[c] over the rows 0 .. n - 1, in a fixed order
hipError_t cox_score_centres(hipStream_t stream, const CoxScoreIn& in, const CoxScoreBufs& b);
// The chain up to Q.  Then, want_rows: sch and score (either may be skipped: want_sch, want_score) become the residuals in the
// caller's ROW order, column c at + c n; want_info: info becomes the m x m matrix.
hipError_t cox_score_run(hipStream_t stream, const CoxPlan& pl, const CoxScoreIn& in, const CoxScoreBufs& b, bool want_sch,
                         bool want_score, bool want_info);
