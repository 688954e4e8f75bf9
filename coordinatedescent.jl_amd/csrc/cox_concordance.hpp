// cox_concordance.hpp -- what the library's translation units share of Harrell's concordance index (cdh_glm_cox_concordance):
// the one launch sequence that cox_concordance.hip defines and cdhip.hip calls (cox_concordance_host.hpp).  A plain function
// over the stream, raw device pointers and the arithmetic of cox_plan.hpp: the handle stays cdhip.hip's.  It returns the first
// error of its launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cox_plan.hpp"

// What the handle holds.  offset, weight and fold are nullptr where the handle has none (fold: k == -1, every row takes part).
struct CoxConcIn {
    const double *y, *r, *offset, *weight;
    const uint8_t* fold;
    int32_t k;
    int64_t n;
};

// the concordance group's scratch, by cox_conc_layout
struct CoxConcBufs {
    const int32_t *order, *qa, *qb;
    double *key0, *v0, *ka, *pa, *kb, *pb, *L, *E, *G, *part, *out;
    int64_t N, tiles;
};

// out[0 .. 3] become the weighted numbers of concordant, discordant and tied pairs among the rows that take part, and the
// number of those rows whose eta is NaN: the tile sort, the fringes, one launch per level from the tile's to the one below
// the top, the rows' products and the fixed-order sum.
hipError_t cox_conc_run(hipStream_t stream, const CoxConcIn& in, const CoxConcBufs& b);
