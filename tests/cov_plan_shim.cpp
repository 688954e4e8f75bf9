// ctypes shim over csrc/cov_plan.hpp (tests/test_cov_plan_host.py builds it with g++ -Wall -Werror: the header holds nothing a
// host compiler cannot take).
#include <cstdlib>
#include <cstring>

#include "../coordinatedescent.jl_amd/csrc/cov_plan.hpp"

// the members of CovSolveBufs the device scratch carries, and those that view the pinned block (CsPinView has them by the same names)
#define CP_DEV_MEMBERS(M)                                                                                                          \
    M(gx) M(bfold) M(bsnap) M(hs) M(newval) M(qs) M(tv) M(pendv) M(ubeta) M(uom) M(ugx) M(uk) M(poff) M(voff) M(uprev) M(iota)      \
    M(touched) M(s2i) M(i2s) M(list) M(vb) M(moved) M(holes) M(fills) M(gxp) M(upos) M(aidx) M(occ) M(setflag) M(inmoved) M(forced) \
    M(colmax) M(Gc) M(gxc) M(cidk) M(gxe) M(cidof) M(ucid) M(newc) M(crew) M(g_snap)
#define CP_PIN_MEMBERS(M) M(in_sup) M(out_sup_idx) M(out_moved_idx) M(out_list) M(out_sup_val) M(out_moved_val)

extern "C" {
int64_t cp_c_const(const char* name) {
#define K(x) if (!std::strcmp(name, #x)) return (int64_t)(x);
    K(kCsThreads) K(kCsLdsBudget) K(kCsLdsFallback) K(kCsUcapMax) K(kCsTrackedMargin) K(kCsTableCap) K(kCsTableMargin) K(kCsTableLds)
    K(kCsTrackedBytes) K(kCsTrackedSlack) K(kCsShuffleMaxP) K(kCsCrewMax)
#undef K
    if (!std::strcmp(name, "sizeof(CovSolveCtl)")) return (int64_t)sizeof(CovSolveCtl);
    if (!std::strcmp(name, "sizeof(CsCrew)")) return (int64_t)sizeof(CsCrew);
    return -1;
}
int64_t cp_c_tri_doubles(int64_t u) { return (int64_t)cs_tri_doubles((size_t)u); }
int64_t cp_c_lds_bytes(int32_t ucap) { return (int64_t)cs_lds_bytes(ucap); }
int32_t cp_c_ucap(int64_t budget) { return cs_ucap((size_t)budget); }
// one plan per support size in nnz[0 .. n): out[9 i ..] = why, ucap, lds_bytes, tcap, nhelp, big, full_cap, fold_limit, nnz_limit
void cp_c_plans(int64_t p, int32_t full, int32_t randomize, int64_t budget, int32_t ucap_limit, int32_t helpers, int32_t big,
                int64_t support_limit, int64_t n, const int64_t* nnz, int64_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        CsPlanIn in{};
        in.p = p; in.nnz = nnz[i]; in.full = full != 0; in.randomize = randomize != 0; in.lds_budget = (size_t)budget;
        in.ucap_limit = ucap_limit; in.helpers = helpers; in.big = big != 0; in.support_limit = support_limit;
        const CsPlan pl = cs_plan(in);
        int64_t* o = out + 9 * i;
        o[0] = pl.why; o[1] = pl.ucap; o[2] = pl.lds_bytes; o[3] = pl.tcap; o[4] = pl.nhelp; o[5] = pl.big ? 1 : 0;
        o[6] = pl.full_cap; o[7] = pl.fold_limit; o[8] = pl.nnz_limit;
        if (pl.run() != (pl.why == kCsRun)) o[0] = -1;
    }
}
int64_t cp_c_dev_bytes(int64_t p) { return (int64_t)cs_dev_bytes((size_t)p); }
int64_t cp_c_pin_bytes(int64_t p) { return (int64_t)cs_pin_layout((size_t)p).bytes; }
// where cs_dev_carve puts member `name` in the scratch (-1: it leaves the member alone, -2: no such member here)
int64_t cp_c_dev_offset(int64_t p, const char* name) {
    char* base = (char*)std::malloc(cs_dev_bytes((size_t)p));
    CovSolveBufs b{};
    cs_dev_carve(b, (size_t)p, base);
    int64_t off = -2;
#define M(x) if (!std::strcmp(name, #x)) off = b.x ? (int64_t)((const char*)b.x - base) : -1;
    CP_DEV_MEMBERS(M)
    CP_PIN_MEMBERS(M)
#undef M
    std::free(base);
    return off;
}
int64_t cp_c_pin_offset(int64_t p, const char* name) {
    char* base = (char*)std::malloc(cs_pin_layout((size_t)p).bytes);
    const CsPinView v = cs_pin_view(base, (size_t)p);
    int64_t off = -2;
    if (!std::strcmp(name, "ctl")) off = (int64_t)((const char*)v.ctl - base);
#define M(x) if (!std::strcmp(name, #x)) off = v.x ? (int64_t)((const char*)v.x - base) : -1;
    CP_PIN_MEMBERS(M)
#undef M
    std::free(base);
    return off;
}
}
