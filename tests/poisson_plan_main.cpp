// poisson_plan_main.cpp -- the record of the Poisson step as the header the kernel and the host share declares it
// (csrc/glm_plan.hpp), compiled with g++ by tests/test_poisson_host.py: its length, and that the plan's records -- one per
// workgroup, whatever the record holds -- times that length stay within what the largest grid asks for.
#include <cstdio>
#include <initializer_list>

#include "glm_plan.hpp"

static_assert(kGlmPoisVals == 6, "nll, sum w, clamped, capped, held-out deviance, training deviance");
static_assert(kGlmPoisVals > kGlmFoldVals && kGlmFoldVals > kGlmVals, "the widest record of the three steps");

int main() {
    const int64_t lds[] = {32, 64, kGlmRows - 32, kGlmRows, kGlmRows + 32, kGlmRows * kGlmMaxGrid, kGlmRows * kGlmMaxGrid + 32,
                           int64_t(1) << 31, (int64_t(1) << 31) + 32};
    for (int64_t ld : lds)
        for (int64_t cap : {kGlmMaxGrid, int64_t(1), int64_t(2), int64_t(0)}) {
            const GlmPlan pl = glm_plan(ld, cap);
            if (pl.records != pl.grid || pl.records < 1 || pl.records * kGlmPoisVals > kGlmMaxGrid * kGlmPoisVals) {
                std::printf("poisson_plan_main FAILED ld=%lld cap=%lld\n", (long long)ld, (long long)cap);
                return 1;
            }
        }
    std::printf("poisson_plan_main OK %d %lld %d\n", kGlmPoisVals, (long long)kGlmMaxGrid, kGlmFoldVals);
    return 0;
}
