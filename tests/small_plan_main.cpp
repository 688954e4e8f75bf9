// Stand-alone check of csrc/small_plan.hpp under the host sanitizers (tests/test_small_plan_host.py builds and runs it):
// for every p in 1 .. 1024 and both LDS budgets, the kernel's dynamic LDS is laid out in an exactly-sized heap block the
// way k_solve_small carves it up and every array is written end to end -- a plan that is too small is an ASan report, an
// unsigned wrap in it a UBSan-visible size -- and the block that crosses the bus is walked the same way.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../coordinatedescent.jl_amd/csrc/small_plan.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static void walk(int64_t p, size_t budget) {
    const SmallPlan pl = small_plan(p, budget);
    const size_t state = small_state_bytes(p);
    EXPECT(pl.fits == (state <= budget));
    if (!pl.fits) { EXPECT(pl.ncache == 0 && pl.lds_bytes == 0); return; }
    EXPECT(pl.ncache >= 0 && pl.ncache <= kSmallMaxCache && pl.lds_bytes <= budget);
    EXPECT(pl.lds_bytes == state + (size_t)pl.ncache * small_col_bytes(p));
    EXPECT(pl.ncache == kSmallMaxCache || pl.lds_bytes + small_col_bytes(p) > budget);      // as many columns as fit
    EXPECT(64 * small_unroll(p) >= p);
    // the kernel's carve-up (k_solve_small), on a heap block of exactly lds_bytes
    char* lds = (char*)std::malloc(pl.lds_bytes);
    double* s_g = (double*)lds;
    double* s_cols = s_g + 4 * p;
    int32_t* s_list = (int32_t*)(s_cols + (size_t)pl.ncache * (size_t)p);
    int32_t* s_fyoff = s_list + 6 * p;
    int32_t* s_fybucket = s_fyoff + p + 1;
    int32_t* s_fypar = s_fybucket + p;
    std::memset(s_g, 1, sizeof(double) * 4 * (size_t)p);
    std::memset(s_cols, 2, sizeof(double) * (size_t)pl.ncache * (size_t)p);
    std::memset(s_list, 3, sizeof(int32_t) * 6 * (size_t)p);
    std::memset(s_fyoff, 4, sizeof(int32_t) * ((size_t)p + 1));
    std::memset(s_fybucket, 5, sizeof(int32_t) * (size_t)p);
    std::memset(s_fypar, 6, sizeof(int32_t) * (size_t)p);
    EXPECT((char*)(s_fypar + p) <= lds + pl.lds_bytes && (char*)(s_fypar + p) + 8 > lds + pl.lds_bytes);
    EXPECT(((char*)s_list - lds) % 8 == 0);
    std::free(lds);
    // [SmallCtl][support][beta]
    const size_t so = small_sup_off(), bo = small_beta_off(p), io = small_io_bytes(p);
    EXPECT(so % 16 == 0 && bo % 16 == 0 && so >= sizeof(SmallCtl) && bo >= so + sizeof(int32_t) * (size_t)p && io == bo + sizeof(double) * (size_t)p);
    char* blk = (char*)std::malloc(io);
    std::memset(blk, 0, sizeof(SmallCtl));
    std::memset(blk + so, 1, sizeof(int32_t) * (size_t)p);
    std::memset(blk + bo, 2, sizeof(double) * (size_t)p);
    std::free(blk);
}

int main() {
    int first_misfit = 0;
    for (int64_t p = 1; p <= kSmallMaxP; ++p) {
        walk(p, kSmallLdsWide);
        walk(p, kSmallLdsDefault);
        EXPECT(small_plan(p, kSmallLdsWide).fits);
        if (!small_plan(p, kSmallLdsDefault).fits && !first_misfit) first_misfit = (int)p;
        if (first_misfit) EXPECT(!small_plan(p, kSmallLdsDefault).fits);
    }
    EXPECT(first_misfit == 964);
    EXPECT(!small_plan(0, kSmallLdsWide).fits && !small_plan(kSmallMaxP + 1, kSmallLdsWide).fits && !small_plan(1, 0).fits);
    EXPECT(small_unroll(256) == 4 && small_unroll(257) == 8 && small_unroll(512) == 8 && small_unroll(513) == 16);
    EXPECT(sizeof(SmallCtl) % 8 == 0 && sizeof(((SmallCtl*)nullptr)->lambdas) == sizeof(double) * kSmallMaxLam);
    std::printf(fails ? "small_plan_main: %d FAILED\n" : "small_plan_main OK\n", fails);
    return fails ? 1 : 0;
}
