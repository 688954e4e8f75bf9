// cov_plan.hpp -- the host-only arithmetic of the device-resident pass loop (cov_solve.hpp: k_cov_solve): the constants that size
// its dynamic LDS, the launch shape and the refusals of one call (cs_plan), and where its arrays lie in the device scratch and in
// the pinned block.  Nothing device-specific in here: tests/test_cov_plan_host.py compiles it with g++ (a shim for ctypes, and a
// stand-alone program under the host sanitizers).  cov_solve() and cs_alloc call these functions and nothing else decides the numbers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "cov_solve_types.hpp"

constexpr int kCsThreads = 256;          // 4 waves, one per SIMD: gram_scalar_body<4> holds a 64-entry Gram column per lane (128 VGPRs) next to the loops' state
constexpr int kCsTrackedMargin = 24;     // room in the tracked list for entering and near-threshold coordinates next to the support
constexpr int kCsTableCap = 1536;        // coordinates the Gram table of large visit lists holds (1536^2 doubles = 18.9 MB of device memory)
constexpr int kCsTableMargin = 160;      // ... of which this many are left to entering and near-threshold coordinates next to the support

// ---- dynamic LDS of k_cov_solve ----------------------------------------------------------------------------------------------
// [G_UU: the Gram block of `ucap` tracked coordinates, upper triangle packed][the tracked arrays].  The kernel carves 84 bytes per
// tracked coordinate behind the block (CsTracked: ten 8-byte arrays and one int32); cs_lds_bytes charges 92.  The 8 more are slack:
// no array stands there.  They stay, because the launch size is cs_lds_bytes and must not change.
// A shuffled pass overlays the whole of it with six (p + 1)-sized int32 arrays; table mode and crew passes overlay the block with
// kCsTableLds doubles.
constexpr size_t kCsLdsBudget = (size_t)134 * 1024;     // asked for, next to ~24 KB of static arrays (160 KB per CU)
constexpr size_t kCsLdsFallback = (size_t)36 * 1024;    // where the runtime refuses that: what the default 64 KB leave next to the static arrays
constexpr int kCsUcapMax = 176;          // where cs_ucap starts looking.  176 itself fits no budget here: its block alone is 176 x 177 / 2
                                         // doubles = 122 KB, 140 800 bytes with the arrays; 172 (134 848 bytes) is the most 134 KB hold
constexpr size_t kCsTrackedBytes = 3 * 8 + 7 * 8 + 4;      // per tracked coordinate, as the kernel carves them
constexpr size_t kCsTrackedSlack = 8;
// (the only function in here the kernel calls: constexpr, which both compilers take on either side)
constexpr size_t cs_tri_doubles(size_t u) { return u * (u + 1) / 2; }
constexpr size_t cs_lds_bytes(int ucap) { return 8 * cs_tri_doubles((size_t)ucap) + (kCsTrackedBytes + kCsTrackedSlack) * (size_t)ucap; }
// the most tracked coordinates a budget of that many bytes holds (in steps of 4, never fewer than 8)
constexpr int cs_ucap(size_t budget) {
    int ucap = kCsUcapMax;
    while (ucap > 8 && cs_lds_bytes(ucap) > budget) ucap -= 4;
    return ucap;
}
// doubles of dynamic LDS table mode and crew passes use: a second block record (GramRec<4>::N rounded up: cov_solve.hpp asserts it),
// a 64 x 64 tile, the two blocks' moves in flight
constexpr size_t kCsTableRec = 2688, kCsTableTile = 64 * 64, kCsTableJobs = 640;
constexpr size_t kCsTableLds = kCsTableRec + kCsTableTile + kCsTableJobs;
constexpr int64_t kCsShuffleMaxP = 5600;    // shuffled sweeps beyond this p are not the loop's: 24 (p + 1) bytes must fit the dynamic LDS

static_assert(cs_ucap(kCsLdsBudget) == 172 && cs_lds_bytes(172) == 134848 && cs_ucap(kCsLdsFallback) == 84, "");
static_assert(cs_lds_bytes(cs_ucap(kCsLdsBudget)) <= kCsLdsBudget && cs_lds_bytes(cs_ucap(kCsLdsFallback)) <= kCsLdsFallback, "");
static_assert(24 * ((size_t)kCsShuffleMaxP + 1) <= cs_lds_bytes(cs_ucap(kCsLdsBudget)), "the shuffle's scratch at the largest p the gate lets through");
static_assert(cs_tri_doubles(cs_ucap(kCsLdsBudget)) >= kCsTableLds, "table mode fits the wide budget");
static_assert(cs_tri_doubles(cs_ucap(kCsLdsFallback)) < kCsTableLds, "... and is off on the fallback");

// ---- the launch shape of one call, and whether there is a launch at all -------------------------------------------------------
enum CsRefusal { kCsRun = 0, kCsSupportBeyondTable, kCsFullBeyondCap, kCsListDoesNotFit, kCsShuffleDoesNotFit };
struct CsPlanIn {
    int64_t p, nnz;              // coordinates, size of the support
    bool full, randomize;
    size_t lds_budget;           // what the runtime granted: kCsLdsBudget or kCsLdsFallback
    int ucap_limit;              // Knobs::cs_ucap
    int helpers; bool big;       // the handle's: helper workgroups a launch may bring, a list has outgrown the LDS block before
    int64_t support_limit;       // the gradient cache's own limit on the support (its policy: the caller computes it)
};
struct CsPlan {
    CsRefusal why;               // kCsRun, or why the pass is the host's
    int ucap; unsigned lds_bytes;
    int32_t tcap;                // 0 or kCsTableCap
    int nhelp; bool big;         // the grid is 1 + nhelp workgroups of k_cov_solve<big>
    int32_t full_cap, fold_limit, nnz_limit;
    bool run() const { return why == kCsRun; }
};
// The LDS of workgroup 0 holds the Gram block of `ucap` tracked coordinates; longer visit lists run from the Gram table, up to its rows.
// Full passes of large supports take g for all p after every block of moves: p x moves gathers per pass, the chip's work and not one
// workgroup's (the bound of the loop's certificates is useless there) -- unless the launch brings helpers, which do it beside the visits.
constexpr CsPlan cs_plan(const CsPlanIn& in) {
    CsPlan pl{};
    pl.ucap = cs_ucap(in.lds_budget);
    pl.lds_bytes = (unsigned)cs_lds_bytes(pl.ucap);
    // (table mode keeps a second block record and a 64 x 64 tile where the LDS Gram block of small lists would be)
    pl.tcap = cs_tri_doubles((size_t)pl.ucap) < kCsTableLds ? 0 : kCsTableCap;
    const int64_t support_cap = kCsTableCap - kCsTableMargin;
    const int ucap_lists = in.ucap_limit > 0 && in.ucap_limit < pl.ucap ? in.ucap_limit : pl.ucap;   // the longest list that runs from the LDS block
    const int lds_margin = kCsTrackedMargin < ucap_lists / 4 ? kCsTrackedMargin : ucap_lists / 4;
    const bool outgrows = in.nnz + lds_margin / 2 > ucap_lists - lds_margin;      // the list is about to leave the LDS block
    const int wanted = in.helpers > 0 && outgrows ? (in.helpers < kCsCrewMax ? in.helpers : kCsCrewMax) : 0;
    pl.full_cap = wanted > 0 ? 0x7fffffff : ucap_lists - lds_margin;
    pl.nhelp = pl.tcap > 0 ? wanted : 0;
    // the instantiation with the large-list paths once a list has outgrown the LDS block on this handle (or is about to: helpers are coming)
    pl.big = pl.tcap > 0 && (in.big || pl.nhelp > 0 || outgrows);
    // a fold is p x (pending moves) gathers: beyond a few moves the chip does it, not the one workgroup of the loop
    pl.fold_limit = (int32_t)(120000 / in.p > 16 ? 120000 / in.p : 16);
    pl.nnz_limit = (int32_t)(in.support_limit < support_cap ? in.support_limit : support_cap);
    pl.why = in.nnz > support_cap ? kCsSupportBeyondTable
           : in.full && in.nnz > pl.full_cap ? kCsFullBeyondCap
           : pl.tcap == 0 && in.nnz > pl.ucap - kCsTrackedMargin ? kCsListDoesNotFit
           : in.randomize && 24 * ((size_t)in.p + 1) > (size_t)pl.lds_bytes ? kCsShuffleDoesNotFit     // its scratch overlays the dynamic LDS
           : kCsRun;
    return pl;
}

// ---- the two layouts ---------------------------------------------------------------------------------------------------------
constexpr size_t cs_align(size_t v) { return (v + 255) / 256 * 256; }

// The device scratch: every array the kernel keeps there, in the order it is carved, as f(member of b, bytes).  The one list:
// cs_dev_bytes and cs_dev_carve both walk it.  (~122 p bytes and the Gram table's 18.9 MB)
template <class F>
void cs_dev_arrays(CovSolveBufs& b, size_t p, F&& f) {
    const size_t tc = (size_t)kCsTableCap;
    auto of = [&](auto*& m, size_t count) { f(m, sizeof(*m) * count); };
    of(b.gx, p); of(b.bfold, p); of(b.bsnap, p); of(b.hs, p); of(b.newval, p); of(b.qs, p); of(b.tv, p); of(b.pendv, p);
    of(b.ubeta, p); of(b.uom, p); of(b.ugx, p);
    of(b.uk, p); of(b.poff, p); of(b.voff, p); of(b.uprev, p); of(b.iota, p);
    of(b.touched, p); of(b.s2i, p); of(b.i2s, p); of(b.list, p); of(b.vb, p); of(b.moved, p); of(b.holes, p); of(b.fills, p);
    of(b.gxp, p); of(b.upos, p); of(b.aidx, p); of(b.occ, p);
    of(b.setflag, p); of(b.inmoved, p); of(b.forced, p);
    of(b.colmax, p);                                                          // M_k of the bound (cs_update_colmax writes it)
    of(b.Gc, tc * tc); of(b.gxc, tc); of(b.cidk, tc); of(b.gxe, tc);          // the Gram table
    of(b.cidof, p); of(b.ucid, p); of(b.newc, p);
    of(b.crew, 1); of(b.g_snap, p);                                           // the crew: jobs, g's snapshot
}
inline size_t cs_dev_bytes(size_t p) {
    CovSolveBufs b{};
    size_t bytes = 0;
    cs_dev_arrays(b, p, [&](auto*&, size_t n) { bytes += cs_align(n); });
    return bytes;
}
// points b's arrays into a block of cs_dev_bytes(p) bytes
inline void cs_dev_carve(CovSolveBufs& b, size_t p, char* base) {
    cs_dev_arrays(b, p, [&](auto*& m, size_t n) { m = reinterpret_cast<std::remove_reference_t<decltype(m)>>(base); base += cs_align(n); });
}

// The pinned block the kernel reads the support from and writes its results into (zero-copy: nothing is copied around the launch):
// [CovSolveCtl][in_sup][out_sup_idx][out_moved_idx][out_list: p int32 each][out_sup_val][out_moved_val: p doubles each]
struct CsPinLayout { size_t in_sup, out_sup_idx, out_moved_idx, out_list, out_sup_val, out_moved_val, bytes; };
constexpr CsPinLayout cs_pin_layout(size_t p) {
    const size_t i = cs_align(4 * p), d = cs_align(8 * p), o = cs_align(sizeof(CovSolveCtl));
    return CsPinLayout{o, o + i, o + 2 * i, o + 3 * i, o + 4 * i, o + 4 * i + d, o + 4 * i + 2 * d};
}
// ... applied to a base: the block as the host addresses it, or as the device does
struct CsPinView {
    CovSolveCtl* ctl = nullptr;
    int32_t *in_sup = nullptr, *out_sup_idx = nullptr, *out_moved_idx = nullptr, *out_list = nullptr;
    double *out_sup_val = nullptr, *out_moved_val = nullptr;
};
inline CsPinView cs_pin_view(char* base, size_t p) {
    const CsPinLayout at = cs_pin_layout(p);
    CsPinView v;
    v.ctl = reinterpret_cast<CovSolveCtl*>(base);
    v.in_sup = reinterpret_cast<int32_t*>(base + at.in_sup);
    v.out_sup_idx = reinterpret_cast<int32_t*>(base + at.out_sup_idx);
    v.out_moved_idx = reinterpret_cast<int32_t*>(base + at.out_moved_idx);
    v.out_list = reinterpret_cast<int32_t*>(base + at.out_list);
    v.out_sup_val = reinterpret_cast<double*>(base + at.out_sup_val);
    v.out_moved_val = reinterpret_cast<double*>(base + at.out_moved_val);
    return v;
}
