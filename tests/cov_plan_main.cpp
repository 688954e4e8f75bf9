// Stand-alone check of csrc/cov_plan.hpp under the host sanitizers (tests/test_cov_plan_host.py builds and runs it): the device
// scratch and the pinned block of the device pass loop are carved out of heap blocks of exactly the computed sizes and every byte
// of every array is written -- a size that is too small is an ASan report -- and the kernel's dynamic LDS is carved the way
// k_cov_solve does it, for both budgets.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../coordinatedescent.jl_amd/csrc/cov_plan.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static void walk_layouts(size_t p) {
    const size_t bytes = cs_dev_bytes(p);
    char* dev = (char*)std::malloc(bytes);
    CovSolveBufs b{};
    cs_dev_carve(b, p, dev);
    size_t written = 0, narrays = 0;
    const char* prev_end = dev;
    cs_dev_arrays(b, p, [&](auto*& m, size_t n) {
        char* at = (char*)const_cast<void*>(static_cast<const void*>(m));
        EXPECT(at >= prev_end && (size_t)(at - dev) % 256 == 0 && at + n <= dev + bytes);
        std::memset(at, (int)(++narrays), n);
        prev_end = at + n; written += n;
    });
    EXPECT(narrays == 41 && prev_end + 256 > dev + bytes && written <= bytes);
    EXPECT(b.g == nullptr && b.Gcols == nullptr && b.slot == nullptr && b.a == nullptr && b.omega == nullptr && b.beta == nullptr && b.in_sup == nullptr);
    std::free(dev);

    const CsPinLayout at = cs_pin_layout(p);
    char* pin = (char*)std::malloc(at.bytes);
    const CsPinView v = cs_pin_view(pin, p);
    std::memset(v.ctl, 0, sizeof(CovSolveCtl));
    std::memset(v.in_sup, 1, 4 * p); std::memset(v.out_sup_idx, 2, 4 * p); std::memset(v.out_moved_idx, 3, 4 * p); std::memset(v.out_list, 4, 4 * p);
    std::memset(v.out_sup_val, 5, 8 * p); std::memset(v.out_moved_val, 6, 8 * p);
    EXPECT((char*)v.out_moved_val + 8 * p <= pin + at.bytes && (char*)v.out_moved_val + 8 * p + 256 > pin + at.bytes);
    EXPECT(v.in_sup[p - 1] == 0x01010101 && v.out_list[0] == 0x04040404);
    std::free(pin);
}

// the kernel's carve of its dynamic LDS (k_cov_solve: the packed Gram block, then CsTracked's arrays), a shuffle's overlay, table mode's
static void walk_lds(size_t budget, int64_t shuffle_p) {
    const int ucap = cs_ucap(budget);
    const size_t bytes = cs_lds_bytes(ucap);
    EXPECT(bytes <= budget && ucap % 4 == 0 && (ucap == kCsUcapMax || cs_lds_bytes(ucap + 4) > budget));
    char* lds = (char*)std::malloc(bytes);
    double* d = (double*)lds + cs_tri_doubles((size_t)ucap);
    std::memset(lds, 1, 8 * cs_tri_doubles((size_t)ucap));
    for (int arr = 0; arr < 10; ++arr) { std::memset(d, 2 + arr, 8 * (size_t)ucap); d += ucap; }
    std::memset(d, 12, 4 * (size_t)ucap);
    EXPECT((char*)d + 4 * (size_t)ucap + kCsTrackedSlack * (size_t)ucap == lds + bytes);      // the slack, and nothing else, is left
    std::memset(lds, 13, 24 * ((size_t)shuffle_p + 1));                                      // six (p + 1)-sized int32 arrays
    if (cs_tri_doubles((size_t)ucap) >= kCsTableLds) std::memset(lds, 14, 8 * kCsTableLds);
    std::free(lds);
}

int main() {
    const size_t ps[] = {1, 16, 17, 255, 256, 257, 1024, 5600, 100003};
    for (size_t p : ps) walk_layouts(p);
    walk_lds(kCsLdsBudget, kCsShuffleMaxP);
    walk_lds(kCsLdsFallback, (int64_t)(cs_lds_bytes(cs_ucap(kCsLdsFallback)) / 24 - 1));
    EXPECT(cs_ucap(0) == 8 && cs_ucap((size_t)1 << 30) == kCsUcapMax);
    CsPlanIn in{};
    in.p = 1000; in.nnz = 10; in.lds_budget = kCsLdsBudget; in.helpers = 31; in.support_limit = 4000;
    EXPECT(cs_plan(in).run() && cs_plan(in).nhelp == 0 && !cs_plan(in).big && cs_plan(in).lds_bytes == 134848);
    in.nnz = kCsTableCap - kCsTableMargin + 1;
    EXPECT(cs_plan(in).why == kCsSupportBeyondTable);
    std::printf(fails ? "cov_plan_main: %d FAILED\n" : "cov_plan_main OK\n", fails);
    return fails ? 1 : 0;
}
