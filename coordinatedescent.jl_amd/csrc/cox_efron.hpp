// cox_efron.hpp -- what the library's two translation units share of the Cox step with Efron ties: the three launches that
// cox_efron.hip defines and cdhip.hip calls between the scans it already has (cox_efron_host.hpp).  Plain functions over the
// stream, raw device pointers and the plan of cox_plan.hpp: the handle stays cdhip.hip's.  Each returns hipGetLastError() of
// its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cox_plan.hpp"

// The scratch of the chain, by cox_layout and cox_efron_layout: the first pair's scans (eT, hA, hB), the runs' sums and head
// flags of the stratum-segmented prefix scans (sums_h: two arrays kCoxMaxGrid apart), and the Efron pair's buffers (Dv follows
// cnt and hc2 follows hc, ld apart; esums: the five arrays of cox_efron_layout).
struct CoxEfronBufs {
    const int32_t *order, *first, *last, *sfirst;
    double *eT, *hA, *hB, *sums_h;
    int32_t* heads_h;
    double *cnt, *Sdv, *hc, *lg, *mm, *esums;
    int32_t *heads_p, *heads_s;
};

// the rows of the handle as k_cox_apply takes them
struct CoxEfronRows {
    const double* status;
    double *y, *r, *w;
    const double* offset;      // or nullptr
    const uint8_t* fold;       // or nullptr: nobody is held out
    int k;
    int64_t n, ld;
    double wmin, eta_max;
    const double* weight;
    double* partials;          // grid records of kCoxVals
};

// after k_cox_exp<true>, before any scan: the inputs of the three tie-group scans and their runs' records
hipError_t cox_efron_mark(hipStream_t stream, const CoxPlan& pl, int64_t ld, const CoxEfronBufs& b);
// after the suffix scan of eT and the three tie-group scans: the four hazard terms, the nll's terms and their runs' records
hipError_t cox_efron_hazard(hipStream_t stream, const CoxPlan& pl, int64_t ld, const CoxEfronBufs& b);
// after the prefix scans of (h, h2) and (hc, hc2): the rows' share and the record's partials
hipError_t cox_efron_apply(hipStream_t stream, const CoxPlan& pl, const CoxEfronBufs& b, const CoxEfronRows& rw, bool apply);
