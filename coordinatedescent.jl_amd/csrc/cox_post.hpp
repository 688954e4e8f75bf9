// cox_post.hpp -- what the library's translation units share of the Cox model's post-estimation exports
// (cdh_glm_cox_residuals, cdh_glm_cox_baseline): the two launch sequences that cox_post.hip defines and cdhip.hip calls
// (cox_post_host.hpp) AFTER the handle's own read-only step, over the scratch that step leaves.  Plain functions over the
// stream, raw device pointers and the plan of cox_plan.hpp: the handle stays cdhip.hip's.  Each returns the first error of its
// launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cox_plan.hpp"

// Which expression forms A of the row at sorted position s: the handle's own chain's.  `last` and `enter` stand for those
// positions moved back to where the table reads hA: the last position of the last tie group at or before them that holds an
// event (cox_post.hip, post_at).
enum class CoxPostChain : int {
    Censored = 0,   // plain and strata: hA[last]
    Interval = 1,   // hA[last] - (enter >= 0 ? hA[enter] : 0)
    Efron = 2,      // an event: (first > sfirst ? hA[first - 1] : 0) + hc[last]; any other row: hA[last]
};

// What the step left and what the handle holds.  A pointer a chain does not have is nullptr: sfirst and hc without Efron, lo,
// enter and T2 without start times, weight and strata on a plain handle (one stratum with id 0, unit weights), offset without one.
struct CoxPostIn {
    const int32_t *order, *first, *last, *sfirst, *lo, *enter;
    const double *eT, *T2, *hA, *hB, *hc;
    const double *status, *y, *r, *offset, *weight, *time;
    const int32_t* strata;
    int64_t n, ld;
    double eta_max;
};

// the post group's scratch, by cox_post_layout
struct CoxPostBufs {
    double *dv, *flag, *out, *sums, *total;
    int32_t *stratum, *slotpos, *heads;
};

// The rows' export, AFTER cox_post_table on the same stream (it reads the scanned flags and slotpos): out + 0, + ld, + 2 ld
// become cumhaz, martingale and deviance in the caller's ROW order, rows 0 .. n - 1; want[i] == false skips that vector's
// stores.
hipError_t cox_post_rows(hipStream_t stream, const CoxPlan& pl, CoxPostChain chain, const CoxPostIn& in, const CoxPostBufs& b,
                         const bool want[3]);
// The baseline table: the tie groups that hold an event, compacted in sorted order into out + c ld (c: time, n_event,
// risk_sum, cumhaz, cumvar) and stratum, the groups' last positions into slotpos; *total becomes their number, as a double.
hipError_t cox_post_table(hipStream_t stream, const CoxPlan& pl, const CoxPostIn& in, const CoxPostBufs& b);
