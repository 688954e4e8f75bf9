// small_plan.hpp -- the host-only arithmetic of the one-launch solve (small_solve.hpp: k_solve_small): the control block the
// kernel exchanges with the host, the bytes of dynamic LDS its p-sized state takes, how many Gram columns fit beside it
// (ncache), which unroll width a p gets, and where the support and beta lie in the block that crosses the bus.  No HIP in
// here: tests/test_small_plan_host.py compiles it with g++ (a shim for ctypes, and a stand-alone program under the host
// sanitizers).  small_prepare and small_solve call these functions and nothing else decides the sizes.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int kSmallMaxP = 1024;
constexpr int kSmallMaxLam = 64;                 // solves per launch (a cold start's numSteps + 1 = 51 by default)

struct SmallCtl {
    double lambdas[kSmallMaxLam];
    int32_t nlam, randomize, loss, has_omega;
    int64_t maxIter;
    double optTol, n_total;
    uint64_t rng;                // splitmix64 state of the substitute RandomIterator: in / out
    int32_t nnz_in, g_from_c;   // g_from_c: `ga` holds (X'y, a) and g = X'y - G beta is formed in the kernel; else ga holds (X'r, a)
    // out
    int64_t passes, full_passes, visits;
    int32_t converged, domain_error;
    double maxH;
    int32_t nnz, precision_lost;
    int64_t steps;               // visit steps taken (each settles a run of positions and makes at most one move)
    uint64_t cycles, ticks;      // shader cycles (s_memtime) and 100 MHz ticks (s_memrealtime) the kernel ran for
};

// ---- dynamic LDS of k_solve_small ------------------------------------------------------------------------------------------
// The p-sized state: four p-vectors of doubles (g, beta, a, omega), nine of int32 (the visit list, the support's slots and
// links, the shuffle and its draws, the column slots, the shuffle's buckets -- whose offsets have p + 1 entries -- their
// contents and the chain pointers), rounded up by the one int32 that keeps the total a multiple of 8.  Then the cached Gram
// columns, p doubles each, which the kernel places between the doubles and the int32 arrays.
constexpr size_t kSmallLdsWide = (size_t)160 * 1024;     // the LDS of one CU (gfx950), where the runtime grants it to a kernel
constexpr size_t kSmallLdsDefault = (size_t)64 * 1024;   // what a kernel gets without asking
constexpr int kSmallMaxCache = 256;                      // Gram columns kept at most

constexpr size_t small_state_bytes(int64_t p) { return (size_t)p * (4 * sizeof(double) + 9 * sizeof(int32_t)) + 2 * sizeof(int32_t); }
constexpr size_t small_col_bytes(int64_t p) { return (size_t)p * sizeof(double); }

struct SmallPlan {
    bool fits;                   // the state alone fits the budget; where it does not, the path switches itself off
    int ncache;                  // Gram columns the kernel can keep beside its state: 0 .. kSmallMaxCache
    unsigned lds_bytes;          // dynamic LDS of the launch: state + ncache columns, <= budget
};
constexpr SmallPlan small_plan(int64_t p, size_t budget) {
    const size_t state = small_state_bytes(p);
    if (p < 1 || p > kSmallMaxP || state > budget) return SmallPlan{false, 0, 0};
    size_t nc = (budget - state) / small_col_bytes(p);
    if (nc > (size_t)kSmallMaxCache) nc = (size_t)kSmallMaxCache;
    return SmallPlan{true, (int)nc, (unsigned)(state + nc * small_col_bytes(p))};
}
// NP of k_solve_small<SQRT, NP>: its loops over a p-vector make NP trips of 64 lanes, so 64 NP >= p
constexpr int small_unroll(int64_t p) { return p <= 256 ? 4 : p <= 512 ? 8 : 16; }
static_assert(64 * small_unroll(kSmallMaxP) >= kSmallMaxP, "the widest kernel covers the largest p");
static_assert(small_plan(kSmallMaxP, kSmallLdsWide).fits && !small_plan(kSmallMaxP, kSmallLdsDefault).fits, "");

// ---- the block that crosses the bus per solve: [SmallCtl][support: p int32][beta: p doubles], each part on 16 bytes --------
constexpr size_t small_sup_off() { return (sizeof(SmallCtl) + 15) / 16 * 16; }
constexpr size_t small_beta_off(int64_t p) { return small_sup_off() + ((size_t)p * sizeof(int32_t) + 15) / 16 * 16; }
constexpr size_t small_io_bytes(int64_t p) { return small_beta_off(p) + (size_t)p * sizeof(double); }
