// quad_solve_types.hpp -- the host-only arithmetic of the batched covariance-form solve (quad_solve.hpp): where a problem's
// state lies in the workgroup's dynamic LDS, how many bytes that takes, the largest p that fits, and the argument checks of
// the cdh_quad exports.  No HIP in here: tests/test_quad_host.py compiles it with g++ into a stand-alone program.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr size_t kQuadLdsBudget = (size_t)160 * 1024;   // the LDS of one CU (gfx950): one problem may take all of it
constexpr int kQuadMaxLam = 64;                         // solves per launch and problem (a cold start's numSteps + 1)
constexpr int kQuadThreads = 64;                        // k_quad_solve's workgroup: one wave (the reason: quad_solve.hpp)

// Byte offsets of the per-problem arrays from the start of dynamic LDS.  Four p-vectors of doubles first (g = A x + b, beta,
// 1 / diag(A), omega), then the int32 arrays k_solve_small keeps (the visit list, the support's slots and links, the shuffle
// and its scratch; the buckets' offsets have p + 1 entries).  No Gram columns are cached: A is read from device memory,
// where all the problems of a batch share it.
struct QuadLds {
    size_t g, beta, inv_a, omega;                                                  // doubles, p each
    size_t list, slot2ind, ind2slot, order, draw, fyoff, fybucket, fypar;          // int32, p each (fyoff: p + 1)
    size_t end;                                                                    // total bytes, a multiple of 8
};
constexpr QuadLds quad_lds_layout(int64_t p) {
    QuadLds L{};
    const size_t d = (size_t)p * sizeof(double), i = (size_t)p * sizeof(int32_t);
    L.g = 0; L.beta = L.g + d; L.inv_a = L.beta + d; L.omega = L.inv_a + d;
    L.list = L.omega + d; L.slot2ind = L.list + i; L.ind2slot = L.slot2ind + i; L.order = L.ind2slot + i;
    L.draw = L.order + i; L.fyoff = L.draw + i; L.fybucket = L.fyoff + i + sizeof(int32_t); L.fypar = L.fybucket + i;
    L.end = (L.fypar + i + 7) / 8 * 8;
    return L;
}
constexpr size_t quad_lds_bytes(int64_t p) { return quad_lds_layout(p).end; }
constexpr int64_t quad_max_p() {                        // the largest p whose state fits the budget (the layout grows with p)
    int64_t p = (int64_t)(kQuadLdsBudget / (4 * sizeof(double) + 8 * sizeof(int32_t)));
    while (p > 0 && quad_lds_bytes(p) > kQuadLdsBudget) --p;
    return p;
}
constexpr int64_t kQuadMaxP = quad_max_p();
static_assert(kQuadMaxP >= 1024, "the issue's floor");
static_assert(quad_lds_bytes(kQuadMaxP) <= kQuadLdsBudget && quad_lds_bytes(kQuadMaxP + 1) > kQuadLdsBudget, "the limit is tight");

// What a problem's solve leaves behind (device memory, one per problem)
struct QuadStat {
    int64_t passes, full_passes, visits;
    int32_t converged, nnz;
    double maxH;                                        // of the last pass
};

// ---- argument checks: a message for what is refused, NULL for what is accepted ---------------------------------------------
inline const char* quad_check_create(int64_t p, int64_t max_batch) {
    if (p <= 0) return "cdh_quad_create: p must be positive";
    if (p > kQuadMaxP) return "cdh_quad_create: p exceeds CDH_QUAD_MAX_P = 2559, the largest problem whose state fits 160 KiB of LDS";
    if (max_batch <= 0 || max_batch > (int64_t)1 << 20) return "cdh_quad_create: max_batch must be in 1 .. 2^20";
    return nullptr;
}
static_assert(kQuadMaxP == 2559, "quad_check_create's message (and CDH_QUAD_MAX_P in cdhip.h) name the limit");
inline const char* quad_check_problem(int64_t j, int64_t m) {
    if (m <= 0) return "no problems are loaded: cdh_quad_set_b first";
    if (j < 0 || j >= m) return "problem index j outside 0 .. m - 1";
    return nullptr;
}
// a support given as (idx1, val): 1-based, inside 1 .. p, no coordinate twice (`seen`: p bytes of scratch, zero on entry and exit)
inline const char* quad_check_support(int64_t p, int64_t nnz, const int64_t* idx1, unsigned char* seen) {
    if (nnz < 0 || nnz > p) return "nnz outside 0 .. p";
    const char* bad = nullptr;
    int64_t s = 0;
    for (; s < nnz; ++s) {
        const int64_t k = idx1[s] - 1;
        if (k < 0 || k >= p) { bad = "a coordinate of the support is outside 1 .. p"; break; }
        if (seen[k]) { bad = "a coordinate appears twice in the support"; break; }
        seen[k] = 1;
    }
    for (int64_t t = 0; t < s; ++t) seen[idx1[t] - 1] = 0;
    return bad;
}
inline const char* quad_check_options(int64_t maxIter, int32_t warmStart, int64_t numSteps) {
    if (maxIter < 0) return "maxIter must not be negative";
    if (!warmStart && (numSteps < 1 || numSteps + 1 > kQuadMaxLam)) return "cold start: numSteps must be in 1 .. 63 (64 solves per launch)";
    return nullptr;
}
