// cdhip.hip -- the C-ABI library (include/cdhip.h): handle, device memory, the pass
// / solve state machine of src/coordinate_descent.jl restated on the host, launches
// of the kernels in kernels.hpp, RCCL row-shard all-reduce.  gfx950 only.
#include "../../include/cdhip.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "kernels.hpp"
#include "gram_kernels.hpp"
#include "vc_kernels.hpp"
#include "vc_gram.hpp"
#include "p2p_exchange.hpp"
#include "sparse_iterate.hpp"
#include "resid_state.hpp"
#include "cache_state.hpp"
#include "exchange_state.hpp"
#include "sweep_plan.hpp"   // the launch shape of the streamed sweep (sweep.hpp) and of the row-summing launches: host-only arithmetic
#include "stats_plan.hpp"   // the launches of a Gram block (col_stats.hpp) and of a varying-coefficient point (vc_host.hpp): host-only arithmetic
#include "solve_plan.hpp"   // the cold start's grid, the screen walk, the gates, where the pass loop stands (solve.hpp): host-only arithmetic

using namespace cdk;

// The batch loop of the column dots (col_dots.hpp: col_dots, col_loadings; vc_point below).  Defined here, by name and value:
// the test suite of the commit before sweep_plan.hpp existed reads the two out of this file when tests/test_gpu_feasible.py is
// imported, and that suite is run unedited against this library.  The plan sizes the partials and the row chunks from its
// restatement, tied below.
constexpr int64_t kColBatch = 4096;   // columns per launch of k_col_dots: keeps the partial buffer small
constexpr int kColChunks = 64;        // row chunks per column in k_col_dots
static_assert(kSpColBatch == kColBatch && kSpColChunks == kColChunks, "sweep_plan.hpp restates the column dots' batch and chunk limits");
static_assert(kSpBlock == kBlock && kSpUnroll == kUnroll && kSpNSum == kNSum && kSpColGroup == kColGroup && kSpGramWaves == kGramWaves,
              "sweep_plan.hpp restates what the kernels fix");
static_assert(sp_gram_rec(1) == GramRec<1>::N && sp_gram_rec(2) == GramRec<2>::N && sp_gram_rec(4) == GramRec<4>::N &&
              sp_block_rec(kMaxBlockB) == BlockRec<kMaxBlockB>::N, "sweep_plan.hpp restates the record sizes");
constexpr bool gram_rec_restated() {
    for (int s = 0; s < kGramLaunchCols; ++s)
        for (int l = s; l < kGramLaunchCols; ++l) if (gs_g(s, l) != GramRec<4>::g(s, l)) return false;
    return kGramLaunchCols == GramRec<4>::B && kGsOffC == GramRec<4>::OFF_C && kGsOffQ == GramRec<4>::OFF_Q && kGsRec == GramRec<4>::N;
}
static_assert(gram_rec_restated(), "stats_plan.hpp restates GramRec<4>");

namespace {

std::string g_create_error;

// ---- RCCL through dlopen: only multi-process runs need it ------------------------
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    void* CommInitRank = nullptr;  // (ncclComm_t*, int nranks, ncclUniqueId by value, int rank)
    int (*CommDestroy)(void*) = nullptr;
    int (*CommAbort)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
struct UniqueId { char bytes[128]; };
typedef int (*comm_init_rank_fn)(void**, int, UniqueId, int);
Rccl g_rccl;

bool load_rccl(std::string& err) {
    if (g_rccl.lib) return true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* nm : names) {
        g_rccl.lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) { err = std::string("dlopen librccl failed: ") + dlerror(); return false; }
    g_rccl.GetUniqueId = (int (*)(void*))dlsym(g_rccl.lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = dlsym(g_rccl.lib, "ncclCommInitRank");
    g_rccl.CommDestroy = (int (*)(void*))dlsym(g_rccl.lib, "ncclCommDestroy");
    g_rccl.CommAbort = (int (*)(void*))dlsym(g_rccl.lib, "ncclCommAbort");
    g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(
        g_rccl.lib, "ncclAllReduce");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(g_rccl.lib, "ncclGetErrorString");
    g_rccl.CommCount = (int (*)(void*, int*))dlsym(g_rccl.lib, "ncclCommCount");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce) {
        err = "librccl is missing ncclGetUniqueId/ncclCommInitRank/ncclAllReduce";
        return false;
    }
    return true;
}
constexpr int kNcclDouble = 8;  // ncclFloat64
constexpr int kNcclSum = 0;

// ---- ownership of the handle's device and pinned host memory -------------------------------------------------------
// A HipBuf owns one allocation and frees it when it goes.  A failed alloc() leaves it empty and clears the runtime's last error
// (the status it returns is the report: a later launch check must not see it again); alloc does nothing else (no memset, no
// synchronisation, no NULL stream).  It reads as the T* it holds.  Moving never frees: a move assignment swaps.
template <class T, bool kPinned>
class HipBuf {
  public:
    HipBuf() = default;
    HipBuf(HipBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    HipBuf& operator=(HipBuf&& o) noexcept { std::swap(p_, o.p_); return *this; }
    ~HipBuf() { if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_)); }
    // (of an empty owner) flags: hipHostMalloc's (pinned), hipExtMallocWithFlags' (device; 0 is plain hipMalloc)
    hipError_t alloc(size_t bytes, unsigned flags = 0) {
        void* q = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&q, bytes, flags)
                                     : flags ? hipExtMallocWithFlags(&q, bytes, flags) : hipMalloc(&q, bytes);
        if (e == hipSuccess) p_ = static_cast<T*>(q);
        else (void)hipGetLastError();
        return e;
    }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    template <class U> explicit operator U*() const { return (U*)p_; }
  private:
    T* p_ = nullptr;
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinBuf = HipBuf<T, true>;

// The captured launch sequences of the chunks (run_chunk), by key: owns their executables.  At most 32: an insert into
// a full cache destroys the oldest.  Entries are found again by key, never kept by pointer across an insert.
struct GraphEntry { uint64_t key; hipGraphExec_t exec; cdh::Captured holds; };
class GraphCache {
  public:
    GraphCache() = default;
    GraphCache(const GraphCache&) = delete;
    GraphCache& operator=(const GraphCache&) = delete;
    ~GraphCache() { clear(); }
    const GraphEntry* find(uint64_t key) const {
        for (const GraphEntry& e : v_) if (e.key == key) return &e;
        return nullptr;
    }
    const GraphEntry* insert(const GraphEntry& e) {
        if (v_.size() >= 32) { (void)hipGraphExecDestroy(v_.front().exec); v_.erase(v_.begin()); }
        v_.push_back(e);
        return &v_.back();
    }
    void clear() {
        for (const GraphEntry& e : v_) (void)hipGraphExecDestroy(e.exec);
        v_.clear();
    }
  private:
    std::vector<GraphEntry> v_;
};

}  // namespace

// Gradient cache of the screened full passes (no reference counterpart; exact).  A visit of a coordinate
// with beta_k == 0 changes nothing unless |X_k'r| exceeds its threshold, and X_k'r is known WITHOUT reading
// X if the Gram columns G_j = X'X_j of every coordinate that moved since a reference point are at hand:
//   X'r = g_ref - sum_j dbeta_j G_j .
// Only the support ever moves, so a handle that keeps solving on the same X (a lambda path, the sigma loop
// of scaledLasso!, the 51 continuation solves of a cold start) pays one pass over X for g_ref, 1.25 passes
// per 32 Gram columns as coordinates enter the support, and after that a full pass costs its exact visits
// only.  Same iterates as visiting one by one: a coordinate is skipped only when the exact path would have
// left it at zero (1e-9 relative margin, as for the dots-only screens), everything else is visited by the
// same kernels.  fp64 storage, no observation weights.
#include "cov_plan.hpp"   // CovSolveCtl, CovSolveBufs (cov_solve_types.hpp) and the host-only arithmetic of the device loop: its launch plan and layouts
struct GradCache {
    int mode = 1;                   // 0 off, 1 rent-or-buy, 2 from the first full pass (both only where the host-side
                                    // fold is cheaper than reading X), 3 from the first full pass, unconditionally
    cdh::CacheState st;             // what is known ABOUT the data below (which copy of g is current, whether g describes r, ...): cache_state.hpp
    int64_t full_seen = 0;          // screened full passes since the data last changed
    int cooldown = 0, backoff = 1;  // after a busy pass: this many full passes run the plain way
    std::vector<double> g, a;
    std::vector<int32_t> slot;      // coordinate -> Gram column, -1 = not cached
    std::vector<std::vector<double>> G;
    DevBuf<double> d_cross;         // device: ceil(p / 64) records of 64 x 32 cross products
    DevBuf<double> d_cross_part;    // device: the same per row-slab block (cross_J of them per column group)
    int cross_J = 1, cross_GX = 1;
    DevBuf<int64_t> d_cols;         // device: the B columns of a batch
    std::vector<double> h_cross;
    // covariance-form visits: device mirrors of g, the Gram columns (slot-major, p doubles each) and the slot map
    bool cov = true;                // covariance-form visits (Knobs::gc_cov; off for good where the store does not fit)
    DevBuf<double> d_g, d_G;
    PinBuf<double> h_g_pin; DevBuf<int32_t> d_slot;
    // whole full passes on the device (gc_pass_device): g lives in d_g between passes and comes back only when host
    // code asks for it (st.host_g_current() / st.dev_g_current() say which copies are current).
    DevBuf<double> d_a, d_g_snap, d_beta_snap, d_qs;
    DevBuf<int64_t> d_pass_idx;           // the pass's visit list (0-based), as uploaded last
    std::vector<int64_t> pass_idx_host;   // ... and what it holds
    DevBuf<int32_t> d_pos_of; int32_t* d_upos = nullptr;
    DevBuf<uint8_t> d_setflag; uint8_t* d_forced = nullptr;   // (d_forced: the second half of d_setflag's allocation)
    int64_t n_forced_rounds = 0;    // full passes of the host's device pass run again with forced coordinates (gc_pass_device)
    // the scan's counters sit at the head of the buffer of unsettled positions (one copy brings both back); the results of
    // a pass come back through k_cov_pack's block
    DevBuf<int32_t> d_scanbuf; PinBuf<int32_t> h_scanbuf;   // [CovScanOut: 4 int32][positions: cap]
    cdk::CovScanOut* d_scan = nullptr;    // = d_scanbuf
    cdk::CovScanOut* h_scan = nullptr;    // = h_scanbuf
    int32_t* h_upos = nullptr;            // = h_scanbuf + 4
    DevBuf<double> d_pack; PinBuf<double> h_pack;           // kPackHead + 2.5 cap doubles
    int64_t n_dev_passes = 0;
    int inject_count = 0;           // device passes so far, for Knobs::gc_inject_rollback (tests)
    int64_t dev_slots_cap = 0, dev_slots = 0;   // columns the device store can hold / holds
    std::vector<DevBuf<double>> d_G_retired;    // stores outgrown on the way (freed with the handle)
    std::vector<double> g_new;      // g as a covariance-form chunk left it, until the chunk is accepted
    int64_t n_rollbacks = 0;
    double drift_last = 0.0, drift_max = 0.0;   // max_k |g_carried - X'r| / thr_k at the re-references so far
    int64_t n_drift = 0;
    int64_t n_validate = 0, n_batches = 0, n_columns = 0, n_certified = 0, n_exact = 0, n_passes = 0, n_cov = 0,
            n_reconcile = 0;
};

// The device-resident pass loop of cache-served solves (cov_solve.hpp): its scratch, the pinned block it reads from and writes
// into, the bound's M_k, its counters.  What a launch looks like is cov_plan.hpp's to say.
struct CovSolvePath {
    bool enabled = true;             // Knobs::cov_solve, cdh_set_device_loop
    bool big = false;                // a visit list has outgrown the loop's LDS block on this handle: launches use the instantiation with the table and the helpers
    int helpers = 31;                // helper workgroups a launch that expects large visit lists brings (Knobs::cs_crew, cdh_set_device_loop; 0: none)
    size_t lds_budget = 0;           // dynamic LDS the runtime grants the kernel (0: not asked yet)
    DevBuf<char> dev; PinBuf<char> pin;   // the scratch and the pinned block: allocated together (cs_alloc), or not at all
    CovSolveBufs bufs{};             // what the kernel gets: the scratch carved, the pinned block as the device addresses it
    CsPinView io;                    // the pinned block as the host addresses it
    CovSolveCtl* ctl_dev = nullptr;  // ... and its head as the device does
    double* colmax = nullptr;        // = bufs.colmax
    int64_t colmax_slots = 0;        // columns of the device store already folded into colmax
    std::vector<double> old;         // scratch: the iterate's values before a launch, by coordinate (zero between launches)
    int32_t tepoch = 0;              // the kernel's Gram table: the epoch of its carried gradients
    int64_t ticks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t n_launches = 0, n_passes = 0, n_folds = 0, n_exact = 0, n_table_passes = 0, n_table_rows = 0;
    int64_t n_forced_rounds = 0, n_crew_passes = 0, n_crew_jobs = 0;
};

// The one-launch solve of problems that fit on chip (small_solve.hpp): the full Gram matrix of the resident X, the
// control block of the solve kernel, pinned staging for what comes back.
#include "small_plan.hpp"   // SmallCtl, kSmallMaxP, kSmallMaxLam; the kernel's LDS plan, unroll width and io offsets: host-only arithmetic
// How much X the Gram form is worth building for is a cost comparison (small_worth_building, small_solve.hpp); X that fits
// kSmallAlwaysBytes takes it regardless (the reference's own test and benchmark shapes).
constexpr size_t kSmallAlwaysBytes = (size_t)16 << 20;

struct SmallPath {
    bool enabled = true;             // Knobs::small_path, cdh_set_small_path
    double rent_paid = 0.0;          // modelled seconds of streamed solves on the current X while G was not built (SmallRent)
    DevBuf<int64_t> d_iota;          // 0 .. p-1: the column lists of the Gram build
    bool G_valid = false;
    DevBuf<double> d_G;              // p x p
    DevBuf<char> d_io; PinBuf<char> h_io;     // [SmallCtl][support][beta]: what crosses the bus per solve, one block each way
    char* hd_io = nullptr;           // h_io as the device addresses it: the kernel works on h_io itself, nothing is copied
    SmallCtl *d_ctl = nullptr, *h_ctl = nullptr;   // views into d_io / h_io (pinned)
    int32_t *d_sup = nullptr, *h_sup = nullptr;
    double *d_beta = nullptr, *h_beta = nullptr;
    int64_t n_solves = 0, n_gram = 0, n_precision = 0;
    bool c_valid = false;            // d_ca / h_c / yy hold X'y (X'Wy), diag(G) and y'y of the current y
    DevBuf<double> d_ca;             // interleaved (c_k, a_k), then y'y at [2p]
    std::vector<double> h_c;         // host copy of c (lambda_max of a cold start needs no device work)
    double yy = 0.0;
    int ncache = 0;                  // Gram columns the solve kernel can keep in LDS
    unsigned lds_bytes = 0;
};

// ---- environment knobs ----------------------------------------------------------------------------------------------
// Every CDH_* variable the library reads (LAB_NOTES.md "Tuning knobs"), read by read_knobs() in cdh_create and kept on the
// handle: a change of the environment reaches the handles created after it, never a live one.  Defaults are the measured
// best.  Where a setting seeds state that the ABI or a fallback changes later (the cache's mode, the device loop, the
// one-launch solve), the handle's state starts from it; the rest is read from here.
constexpr int64_t kGcCovRefresh = 200000;   // covariance-form visits after which g is re-read from X
// The scratch of cdh_vc_gram and cdh_vc_gram_batch besides the handle's data (vc_gram.hpp), in two tiers, each allocated together
// by the first call that needs it, or not at all.  Who owns what:
//   VcGramScratch       the first call of either export.  Its input block (the listed columns with one point behind them: one copy
//                       takes both to the device) and e serve both exports; partials (16 MiB), out and h_out (one summed record) and
//                       the block's point are cdh_vc_gram's alone, so a handle that never calls the batch allocates no more.
//   VcGramBatchScratch  the first cdh_vc_gram_batch (vc_gram_batch_types.hpp: vgb_scratch_*_bytes): the partial records of a launch
//                       group, its summed records on the device and pinned, and the group's points.
// vc_gram_run works in a VcGramBufs: the five buffers in which the tiers differ.
struct VcGramInput { int64_t cols[kVgMaxCols]; VcGramPoint pt; };
struct VcGramScratch {
    DevBuf<double> partials, out;
    DevBuf<VcGramInput> in;
    DevBuf<void> e;
    PinBuf<double> h_out;
    PinBuf<VcGramInput> h_in;
    bool ready = false;
};
struct VcGramBatchScratch {
    DevBuf<double> partials, out;
    DevBuf<VcGramPoint> pts;
    PinBuf<double> h_out;
    PinBuf<VcGramPoint> h_pts;
    bool ready = false;
};
struct VcGramBufs { double *partials, *out, *h_out; VcGramPoint *pts, *h_pts; };

// Cross-validation folds (cv_path.hpp).  The fold ids of the rows -- a byte each, resident from cdh_set_folds until it drops them
// -- and the scratch of cdh_path_sse, allocated by its first call: the workgroups' partial records, the summed record, the
// 0-based coordinates of a call and the packed image of its B (cv_plan.hpp: sizes and layouts; the image grows with the calls).
#include "cv_plan.hpp"
struct CvState {
    DevBuf<uint8_t> fold;
    int K = 0;                 // 0: no folds set
    DevBuf<double> partials, out, B;
    DevBuf<int64_t> idx;
    int64_t b_cap = 0;
    bool ready = false;
};

// The logistic loss (glm_kernels.hpp): the labels of the rows, resident from cdh_glm_set_labels on in a buffer of the handle's
// own -- y holds the working response of the IRLS round, not the labels.  glm_plan.hpp: the grid and the rows of a workgroup.
#include "glm_plan.hpp"
#include "cox_plan.hpp"   // the Cox step's tiles, runs and scratch layout; the time order and its tie groups: host-only arithmetic
#include "cox_efron.hpp"  // the three launches of the Efron chain that the second translation unit (cox_efron.hip) defines
#include "cox_post.hpp"   // the post-estimation exports' launches that the third translation unit (cox_post.hip) defines
#include "cox_concordance.hpp"   // the concordance index's launches that the fourth translation unit (cox_concordance.hip) defines
#include "cox_score.hpp"   // the score residuals' and the information matrix's launches that the fifth translation unit (cox_score.hip) defines
enum class GlmData : int { Binomial = 0, Poisson = 1, Cox = 2 };
// The Cox group (cox_kernels.hpp; cox_layout): d -- the scans' scratch, the runs' sums and the times; i -- order and the tie
// groups' bounds.  Allocated together by the first cdh_glm_set_survival, or not at all.  sd, si -- the second pair, of a handle
// with strata or observation weights: allocated together by the first cdh_glm_set_survival_strata that brings either, and in
// use while `strata` is set (every other setter of observations clears it).  vd, vi -- the third pair, of a handle with start
// times: allocated together by the first cdh_glm_set_survival_interval that brings them, and in use while `interval` is set
// (then `strata` is set too; every setter without start times clears it).  ed, ei -- the Efron pair (cox_efron_layout), of a
// handle set to Efron ties: allocated together by the first cdh_glm_set_cox_ties that asks for them, and in use while `efron`
// is set (then `strata` is set too: the Efron chain is segmented and weighted; a setter with start times, the label and the
// count setters clear it).  pd, pi -- the post group (cox_post_layout), of a handle that was asked for residuals or a baseline
// hazard: allocated together by the first cdh_glm_cox_residuals or cdh_glm_cox_baseline, scratch of those calls alone.
// cd, ci -- the concordance group (cox_conc_layout): allocated together by the first cdh_glm_cox_concordance, which also fills
// its order; every setter of survival data drops it, since the order is the data's.  qd, qi -- the score group
// (cox_score_layout) for score_cols columns: allocated together by the first cdh_glm_cox_score and regrown together, never
// shrunk, when a later call asks for more columns; scratch of that call alone, which fills it anew every time.
struct CoxState {
    DevBuf<double> d;
    DevBuf<int32_t> i;
    DevBuf<double> sd;
    DevBuf<int32_t> si;
    DevBuf<double> vd;
    DevBuf<int32_t> vi;
    DevBuf<double> ed;
    DevBuf<int32_t> ei;
    DevBuf<double> pd;
    DevBuf<int32_t> pi;
    DevBuf<double> cd;
    DevBuf<int32_t> ci;
    DevBuf<double> qd;
    DevBuf<int32_t> qi;
    int64_t score_cols = 0;
    bool strata = false;
    bool interval = false;
    bool efron = false;
};
struct GlmState {
    DevBuf<double> labels;     // the labels, or the counts of the Poisson family
    DevBuf<double> offset;     // Poisson: ld doubles, pads zero; allocated by the first cdh_glm_set_counts that brings one
    GlmData family = GlmData::Binomial;   // what `labels` holds: cdh_glm_set_labels' labels or cdh_glm_set_counts' counts
    bool has_offset = false;   // the offset buffer holds this handle's offset (false: the step runs without one)
    DevBuf<double> prior;      // binomial and Poisson: the observation weights v, ld doubles, pads zero; allocated by the
                               // first cdh_glm_set_weights that brings them, in use while `weighted` is set
    bool weighted = false;     // the step runs its weighted instantiation (every setter of observations clears it)
    bool set = false;
    CoxState cox;              // GlmData::Cox: `labels` holds the status, `offset` the offset
};

struct Knobs {
    int lt = 2;                      // CDH_LT: k_gramstep's operand loads transposed through LDS: 0 off, 1 on, 2 by size
    int ks = 0;                      // CDH_KS: chunk length of that path: 0 by shard length, 1 short, 2 long
    int gradient_cache = 1;          // CDH_GRADIENT_CACHE: the cache's initial mode (0 - 3)
    bool gc_cov = true;              // CDH_GC_COV: covariance-form visits
    int64_t gc_refresh = kGcCovRefresh;    // CDH_GC_REFRESH (tests)
    int gc_inject_rollback = 0;      // CDH_GC_INJECT_ROLLBACK (tests): every N-th device pass of the cache is declared failed
    int64_t gc_rows_per_nnz = 0;     // CDH_GC_ROWS_PER_NNZ (tests): a fixed rows-per-non-zero rule (0: by path, gc_rows_per_nnz)
    bool cov_solve = true;           // CDH_COV_SOLVE: the device-resident pass loop
    int cs_crew = 31;                // CDH_CS_CREW: its helper workgroups (0: none)
    int cs_ucap = 0;                 // CDH_CS_UCAP (tests): visit lists longer than this leave the loop's LDS block
    int64_t glm_grid = kGlmMaxGrid;  // CDH_GLM_GRID (tests): cap of k_glm_step's grid, so that a short vector gives a workgroup a second stride
    int64_t cox_grid = kCoxMaxGrid;  // CDH_COX_GRID (tests): cap of the Cox step's grid, so that a few thousand rows give a workgroup several tiles
    bool small_path = true;          // CDH_SMALL_PATH: the one-launch solve
    int64_t small_max_bytes = -1;    // CDH_SMALL_MAX_BYTES: a fixed limit on n p sz instead of rent-or-buy (-1: none)
    int64_t small_always_bytes = (int64_t)kSmallAlwaysBytes;   // CDH_SMALL_ALWAYS_BYTES (tests: 0 makes every handle rent first)
    bool force_rccl = false;         // CDH_FORCE_RCCL (set): cdh_comm_init builds a 1-rank communicator too
    unsigned p2p_spin_limit = cdk::kP2PSpinLimit;   // CDH_P2P_SPIN_LIMIT: bound of the direct exchange's wait
};

// the only reader of the environment in the library
Knobs read_knobs() {
    auto num = [](const char* nm, long long dflt) { const char* v = getenv(nm); return v ? atoll(v) : dflt; };
    Knobs k;
    k.lt = (int)num("CDH_LT", k.lt);
    k.ks = (int)num("CDH_KS", k.ks);
    k.gradient_cache = (int)std::max(0LL, std::min(3LL, num("CDH_GRADIENT_CACHE", k.gradient_cache)));
    k.gc_cov = num("CDH_GC_COV", 1) != 0;
    k.gc_refresh = std::max(1LL, num("CDH_GC_REFRESH", k.gc_refresh));
    k.gc_inject_rollback = (int)std::max(0LL, num("CDH_GC_INJECT_ROLLBACK", 0));
    if (getenv("CDH_GC_ROWS_PER_NNZ")) k.gc_rows_per_nnz = std::max(1LL, num("CDH_GC_ROWS_PER_NNZ", 1));
    k.cov_solve = num("CDH_COV_SOLVE", 1) != 0;
    k.cs_crew = (int)std::max(0LL, std::min((long long)kCsCrewMax, num("CDH_CS_CREW", k.cs_crew)));
    k.cs_ucap = (int)std::max(0LL, num("CDH_CS_UCAP", 0));
    k.glm_grid = glm_grid_cap(num("CDH_GLM_GRID", k.glm_grid));
    k.cox_grid = cox_grid_cap(num("CDH_COX_GRID", k.cox_grid));
    k.small_path = num("CDH_SMALL_PATH", 1) != 0;
    k.small_max_bytes = num("CDH_SMALL_MAX_BYTES", k.small_max_bytes);
    k.small_always_bytes = num("CDH_SMALL_ALWAYS_BYTES", k.small_always_bytes);
    k.force_rccl = getenv("CDH_FORCE_RCCL") != nullptr;
    k.p2p_spin_limit = (unsigned)std::max(1LL, num("CDH_P2P_SPIN_LIMIT", k.p2p_spin_limit));
    return k;
}

// cdh_profile_begin / cdh_profile_end: device time, launches and algorithmic bytes of the brackets in between.  A bracket is
// begin(), its launches, stop() -- both in stream order -- and, once the stream has been synchronised, end() with what it counts.
struct Profile {
    bool on = false;
    double ms = 0.0, bytes = 0.0;
    int64_t launches = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t begin(hipStream_t s) const { return on ? hipEventRecord(ev0, s) : hipSuccess; }
    hipError_t stop(hipStream_t s) const { return on ? hipEventRecord(ev1, s) : hipSuccess; }
    hipError_t end(int64_t its_launches, double its_bytes) {
        if (!on) return hipSuccess;
        float t = 0.f;
        const hipError_t e = hipEventElapsedTime(&t, ev0, ev1);
        if (e != hipSuccess) return e;
        ms += t; launches += its_launches; bytes += its_bytes;
        return hipSuccess;
    }
};

struct cdh_handle_s {
    int dtype = CDH_F64, loss = CDH_LS, device = 0;
    int64_t n = 0, n_total = 0, row0 = 0, p = 0, ld = 0, nvec = 0;
    size_t esz = 8;
    hipStream_t stream = nullptr;
    // device
    DevBuf<void> X, y, r, w;
    // varying-coefficient mode (cdh_vc_set_data): z, typed as X; base column j of the design sits at column j (vc_degree + 1)
    DevBuf<void> vc_z;
    int64_t vc_pbase = 0;
    int vc_degree = -1;           // -1: not in varying-coefficient mode
    VcGramScratch vg;
    VcGramBatchScratch vgb;
    CvState cv;
    GlmState glm;
    DevBuf<double> beta, omega;
    DevBuf<Ctrl> d_ctrl;
    DevBuf<int64_t> d_idx;
    DevBuf<double> d_hs, d_newval;
    DevBuf<int32_t> d_touched;
    DevBuf<double> d_partials, d_red, d_colout;
    DevBuf<int64_t> d_sup_idx;
    DevBuf<double> d_sup_val;
    // pinned host staging
    PinBuf<int64_t> h_idx;
    PinBuf<double> h_hs, h_newval, h_red;
    PinBuf<int32_t> h_touched;
    PinBuf<Ctrl> h_ctrl;
    // state
    int64_t cap = 0;          // visits per chunk
    SweepSizes sz{};          // what cdh_create derived (sweep_plan.hpp): the fixed grids, the CU count, the doubles of d_partials; ld, nvec and cap above are its
    Ctrl ctrl{};
    bool has_omega = false, has_w = false, y_set = false;
    std::vector<double> h_omega;  // host copy of the penalty weights (thresholds, objective)
    bool omega_dev_ok = false;    // the device's omega holds h_omega
    cdh::SupportList x;
    int mode = CDH_SWEEP_BLOCK, blockB = 32;   // the default (cdh_create: 64 on short fp64 columns); cdh_set_sweep_mode changes it
    // The default width is chosen from the rank-LOCAL row count, and near-equal row shards can fall on opposite sides of the
    // cut (n_total = 524287 over two ranks: 262144 and 262143 rows) -- ranks with different B would issue different numbers
    // and sizes of all-reduces per pass.  So a sharded handle that still has its default agrees on it through the exchange
    // before its first streamed chunk (agree_default_width): 64 only if every rank chose 64.
    bool width_default = true, width_agreed = false;
    bool use_graph = false;
    int screening = 1;            // 0 never, 1 the solves' full passes over sparse iterates, 2 cdh_pass too
    bool reuse_residual = false;  // warm starts skip initialize! when r is known to match beta
    cdh::ResidState rs;           // what r holds and stands for, the moves it owes, the stashed dots (resid_state.hpp)
    bool chunk_dup = false;       // the current chunk's visit list repeats a coordinate
    std::vector<int32_t> stamp;   // duplicate detection scratch, size p
    GraphCache graphs;               // captured chunk launch sequences
    bool graph_broken = false;       // a capture failed on this handle: launch node by node from now on
    bool domain_error = false;
    Knobs knobs;    // the environment as cdh_create found it
    // the row-shard exchange: who serves it, where an all-reduce goes, epochs, capture bookkeeping (exchange_state.hpp) ...
    cdh::ExchangeState xs;
    // ... and the HIP resources behind it.  The optional direct exchange of the short records (p2p_exchange.hpp):
    DevBuf<unsigned long long> p2p_inbox;
    cdk::P2PPeers p2p_peers{};
    std::vector<void*> p2p_mapped;
    PinBuf<int> p2p_timeout;     // pinned host flag written by a kernel whose bounded spin ran out
    DevBuf<unsigned> d_p2p_base;      // epoch base of a replayed graph's exchanges (device memory)
    // bring-your-own transport (cdh_set_host_exchange): staged through pinned host memory
    PinBuf<double> h_xchg;
    size_t h_xchg_doubles = 0;
    // profile
    GradCache gc;
    CovSolvePath cs;
    SmallPath small;
    Profile prof;
    std::string err;
};

// ---- the second handle: a batch of CDQuadraticLoss problems on one A (quad_solve.hpp) ----------------------------------------
#include "quad_solve_types.hpp"   // the LDS layout, CDH_QUAD_MAX_P's formula, the argument checks: host-only arithmetic
static_assert(kQuadMaxP == CDH_QUAD_MAX_P, "cdhip.h names the limit quad_solve_types.hpp derives");
struct cdh_quad_s {
    int64_t p = 0, max_batch = 0, m = 0;   // m: the problems loaded by the last cdh_quad_set_b
    int32_t device = 0;
    hipStream_t stream = nullptr;
    unsigned lds_bytes = 0;
    bool A_set = false, penalty_set = false, has_omega = false, omega_shared = false;
    // device: A (p x p), 1 / diag(A); per problem b, omega, lambda0 and a cold start's grid, beta (dense), g = A x + b, the
    // support in slot order and its length, the statistics; the explicit list of cdh_quad_pass and a descent's h
    DevBuf<double> A, inv_a, B, omega, lambda0, grid, beta, g, h_out;
    DevBuf<int32_t> sup, nnz, list;
    int64_t list_cap = 0;
    DevBuf<QuadStat> stats;
    PinBuf<QuadStat> h_stats;
    PinBuf<double> h_h;
    // host: what lambda_max of a cold start is taken from, and the iterates as last fetched (host_stale: the device has moved on)
    std::vector<double> h_B, h_omega, h_lambda0, h_beta;
    std::vector<int32_t> h_sup, h_nnz;
    bool host_stale = true;
};

namespace {

#define HIPCHK(h, call)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            char buf_[512];                                                                 \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                   \
            (h)->err = buf_;                                                                \
            return e_ == hipErrorOutOfMemory ? CDH_OOM : CDH_HIP_ERROR;                     \
        }                                                                                   \
    } while (0)

#define CHK(call)                                   \
    do {                                            \
        int32_t s_ = (call);                        \
        if (s_ != CDH_OK) return s_;                \
    } while (0)

int32_t fail(cdh_handle h, int32_t code, const char* msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

// every export checks what it dereferences: a NULL handle (guarded, below) or out-pointer is CDH_BAD_ARG, never a crash
#define NEED_P(h, ptr)                                                         \
    do {                                                                       \
        if (!(ptr)) return fail((h), CDH_BAD_ARG, #ptr " is NULL");            \
    } while (0)

template <typename F> int32_t dispatch(cdh_handle h, F&& f) {
    return h->dtype == CDH_F64 ? f((double*)nullptr) : f((float*)nullptr);
}

int32_t upload_ctrl(cdh_handle h) {
    *h->h_ctrl = h->ctrl;
    HIPCHK(h, hipMemcpyAsync(h->d_ctrl, h->h_ctrl, sizeof(Ctrl), hipMemcpyHostToDevice, h->stream));
    return CDH_OK;
}

// what the exchange's state refuses is the export's error (exchange_state.hpp)
inline int32_t refused(cdh_handle h, const cdh::Refusal& r) { return r.status == CDH_OK ? (int32_t)CDH_OK : fail(h, r.status, r.msg); }
int32_t exchange_alive(cdh_handle h) { return refused(h, h->xs.alive()); }
// has a kernel of the direct exchange run out of its bounded spin?
int32_t p2p_check(cdh_handle h) {
    if (h->xs.direct_on() && *(volatile int*)h->p2p_timeout) return refused(h, h->xs.p2p_timed_out());
    return CDH_OK;
}

static_assert(GramRec<4>::N <= cdk::kP2PMaxCount, "the widest block record must fit one inbox slot");
// the arguments of the next direct exchange.  While a graph is being recorded the epoch is
// (device-resident base) + (position of the exchange in the graph), so one graph serves every replay.
cdk::P2PCall next_p2p_call(cdh_handle h) {
    cdh::ExchangeState& xs = h->xs;
    return cdk::P2PCall{h->p2p_peers, xs.rank(), xs.direct_ranks(), xs.next_epoch(), h->knobs.p2p_spin_limit, h->p2p_timeout,
                        xs.in_capture() ? (const unsigned*)h->d_p2p_base : nullptr};
}

// The one exchange seam of the row-sharded path: sum `count` doubles at dbuf (device) over all ranks,
// in stream order.  Behind it: the direct exchange (short records), RCCL, or a caller-supplied host
// transport.  Not sharded: nothing to do.
int32_t allreduce(cdh_handle h, double* dbuf, size_t count) {
    cdh::ExchangeState& xs = h->xs;
    const cdh::Routing to = xs.route(count);
    switch (to.route) {
    case cdh::Route::Refuse: return refused(h, to.why);
    case cdh::Route::Nothing: return CDH_OK;
    case cdh::Route::Host:
        for (size_t o = 0; o < count; o += h->h_xchg_doubles) {   // long records go through the staging buffer in pieces
            const size_t cnt = std::min(h->h_xchg_doubles, count - o);
            HIPCHK(h, hipMemcpyAsync(h->h_xchg, dbuf + o, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            const int32_t rc = xs.host_callback()(xs.host_context(), h->h_xchg, (int64_t)cnt);
            if (rc != 0) return fail(h, CDH_RCCL_ERROR, "the host exchange callback reported a failure");
            HIPCHK(h, hipMemcpyAsync(dbuf + o, h->h_xchg, sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));   // the staging buffer is reused by the next exchange
        }
        break;
    case cdh::Route::Direct:
        CHK(p2p_check(h));
        for (size_t o = 0; o < count; o += cdk::kP2PMaxCount) {
            const int c = (int)std::min<size_t>(cdk::kP2PMaxCount, count - o);
            hipLaunchKernelGGL(cdk::k_p2p_allreduce, dim3((c + 255) / 256), dim3(256), 0, h->stream, dbuf + o, c,
                               next_p2p_call(h));
            xs.issued(to.route);
        }
        HIPCHK(h, hipGetLastError());
        return CDH_OK;
    case cdh::Route::Rccl: {
        const int rc = g_rccl.AllReduce(dbuf, dbuf, count, kNcclDouble, kNcclSum, xs.communicator(), h->stream);
        if (rc != 0) {
            h->err = std::string("ncclAllReduce failed: ") +
                     (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
            return CDH_RCCL_ERROR;
        }
        break;
    }
    }
    xs.issued(to.route);   // host, RCCL: once per all-reduce that went through
    return CDH_OK;
}

// ---- r catches up with the covariance-form visits: r -= sum_k pending_k X_k, 64 columns per launch ----------
// Called by everything that reads r -- the streaming kernels, the dots, the moments, the Gram entry point, the
// download (cdh_get_residual) -- and before X itself changes; nothing else needs r, so a warm-started path
// whose solves all run from the cache pays for one catch-up when its caller finally asks for the residual
// (moves of the same coordinate merge in the meantime).
// (declared ahead, not moved above: where sync_r stands decides the order in which the kernel templates are first used, and
// with it the order of the kernels in the code object -- kept as it was, so that the device code is unchanged)
int32_t rebuild_residual_from(cdh_handle h, const cdh::SupportList& x, bool with_beta);
int32_t sync_r(cdh_handle h) {
    cdh::ResidState& rs = h->rs;
    if (rs.lazy()) return rebuild_residual_from(h, rs.take_lazy(), false);   // (beta on the device mirrors h->x: left alone)
    if (rs.pending().empty()) return CDH_OK;
    rs.catchup_begins();
    const cdh::MoveLedger& L = rs.pending();
    for (size_t o = 0; o < L.size(); o += 64) {
        const int cnt = (int)std::min<size_t>(64, L.size() - o);
        for (int i = 0; i < cnt; ++i) { h->h_idx[i] = L[o + (size_t)i]; h->h_hs[i] = L.value(L[o + (size_t)i]); }
        HIPCHK(h, hipMemcpyAsync(h->d_idx, h->h_idx, sizeof(int64_t) * (size_t)cnt, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_hs, h->h_hs, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, h->stream));
        CHK(dispatch(h, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            hipLaunchKernelGGL(k_multi_axpy<T>, dim3(h->sz.step_grid), dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld,
                               h->nvec, (T*)h->r, h->d_idx, h->d_hs, 0, cnt);
            return CDH_OK;
        }));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->stream));   // the pinned staging arrays are reused
        rs.catchup_batch_applied();
    }
    rs.catchup_done();
    h->gc.n_reconcile += 1;
    return CDH_OK;
}

#include "col_dots.hpp"   // need_partials; col_dots, col_loadings, resid_moments_dev

// ---- gradient cache: bookkeeping (its constants, its admission and its passes: grad_cache.hpp) ------------------------
// g no longer describes r (y or the loss changed); with `columns` the Gram columns are gone too (X changed)
void gc_invalidate(cdh_handle h, bool columns) {
    GradCache& c = h->gc;
    c.st.invalidated(columns);
    if (columns) {
        c.G.clear(); c.G.shrink_to_fit();
        std::fill(c.slot.begin(), c.slot.end(), -1);     // (d_slot still names the old columns until the next upload)
        h->cs.colmax_slots = 0;
        c.dev_slots = 0;                 // the device store is refilled from slot 0 (its memory is kept)
        c.full_seen = 0;
    }
}
// r was just set to y - X * (the handle's iterate) by a kernel
void gc_after_rebuild(cdh_handle h, const cdh::SupportList& x) { h->gc.st.rebuilt(x, h->p); }
// the streamed visits of a chunk have updated r: g learns of them at the next fold
void gc_note_moves(cdh_handle h, const int64_t* idx0, int m) {
    for (int i = 0; i < m; ++i)
        if (h->h_hs[i] != 0.0 && !h->gc.st.moved(idx0[i], h->h_hs[i], cdh::MoveKind::streamed)) return;
}

// ---- initialize!: upload support, r = y - X beta ------------------------------------
// the dense beta of x goes to the device (nothing host-side stays in flight)
int32_t upload_beta(cdh_handle h, const cdh::SupportList& x) {
    if (x.nnz() == 0) {
        HIPCHK(h, hipMemsetAsync(h->beta, 0, sizeof(double) * h->p, h->stream));
        return CDH_OK;
    }
    std::vector<double> dense((size_t)h->p, 0.0);
    for (int64_t s = 0; s < x.nnz(); ++s) dense[(size_t)x.coord(s)] = x.slot_value(s);
    HIPCHK(h, hipMemcpyAsync(h->beta, dense.data(), sizeof(double) * h->p, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // `dense` goes out of scope
    return CDH_OK;
}
int32_t rebuild_residual_from(cdh_handle h, const cdh::SupportList& x, bool with_beta) {
    if (h->rs.rebuild_is_noop(x)) {   // the buffer already holds exactly what this rebuild would write
        if (with_beta) CHK(upload_beta(h, x));
        h->rs.rebuild_skipped();
        gc_after_rebuild(h, x);
        return CDH_OK;
    }
    h->rs.rebuild_begins();           // r = y - X beta, summed in fp64 and rounded once
    if (with_beta) CHK(upload_beta(h, x));
    const int64_t nnz = x.nnz();
    if (nnz == 0) {   // the cold start: beta = 0, r = y; nothing host-side is in flight, so no wait either
        HIPCHK(h, hipMemcpyAsync(h->r, h->y, (size_t)h->ld * h->esz, hipMemcpyDeviceToDevice, h->stream));
    } else {
        std::vector<int64_t> si((size_t)nnz);
        std::vector<double> sv((size_t)nnz);
        for (int64_t s = 0; s < nnz; ++s) { si[(size_t)s] = x.coord(s); sv[(size_t)s] = x.slot_value(s); }
        HIPCHK(h, hipMemcpyAsync(h->d_sup_idx, si.data(), sizeof(int64_t) * nnz, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_sup_val, sv.data(), sizeof(double) * nnz, hipMemcpyHostToDevice, h->stream));
        const int grid = elementwise_grid(h->nvec, kInitGridCap);
        CHK(dispatch(h, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            hipLaunchKernelGGL(k_init_resid<T>, dim3(grid), dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld,
                               h->nvec, (const T*)h->y, (T*)h->r, h->d_sup_idx, h->d_sup_val, (int)nnz);
            return CDH_OK;
        }));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->stream));  // host vectors above go out of scope
    }
    h->rs.rebuilt_from(x);
    gc_after_rebuild(h, x);
    return CDH_OK;
}
int32_t rebuild_residual(cdh_handle h) { return rebuild_residual_from(h, h->x, true); }

#include "sweep.hpp"   // note_duplicates, finish_chunk, the three launchers of a chunk, run_chunk

#include "grad_cache.hpp"   // gc_size, gc_validate, gc_fetch, gc_fold, gc_full_pass
#include "small_solve.hpp"  // small_applicable, small_prepare, small_solve
#include "cov_solve.hpp"    // k_cov_solve, cov_solve: the pass loop of a cache-served solve on the device
#include "quad_solve.hpp"   // k_quad_solve, k_quad_init: a batch of CDQuadraticLoss problems, one workgroup each
#include "cv_path.hpp"      // k_fold_weights, k_path_sse: the folds of a cross-validated path and its errors in one pass
#include "glm_kernels.hpp"  // k_glm_step: the step between two IRLS rounds of a GLM family
#include "cox_kernels.hpp"  // the Cox family's step: risk-set scans in time order, a chain of launches
#include "cox_post_host.hpp"  // residuals and the baseline hazard of a fitted Cox model: host bodies, the kernels are cox_post.hip's
#include "cox_concordance_host.hpp"  // Harrell's concordance index: the host body, the kernels are cox_concordance.hip's
#include "cox_score_host.hpp"  // score and Schoenfeld residuals, the information matrix: the host body, the kernels are cox_score.hip's

#include "solve.hpp"       // screened_full_pass, run_pass, solve; the bodies of cdh_descend, cdh_pass, cdh_solve, cdh_coordinate_descent

void free_all(cdh_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->xs.communicator() && g_rccl.CommDestroy) g_rccl.CommDestroy(h->xs.communicator());
    for (void* m : h->p2p_mapped) (void)hipIpcCloseMemHandle(m);
    const hipEvent_t ev[] = {h->prof.ev0, h->prof.ev1};
    const hipStream_t stream = h->stream;
    delete h;   // the owners free the device and pinned memory and the captured graphs, before the stream goes
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
}

// ---- exception firewall: nothing may unwind across the C ABI -------------------------------------
// Every export that returns a status runs its body through here.  Without a handle (cdh_create, cdh_destroy, cdh_device_count,
// cdh_comm_unique_id) the message goes where cdh_last_error(NULL) finds it.
template <typename F> int32_t guarded_as(cdh_handle h, F&& body) {
    try { return body(); }
    catch (const std::bad_alloc&) { return fail(h, CDH_OOM, "host allocation failed"); }
    catch (const std::exception& e) { return fail(h, CDH_BAD_ARG, e.what()); }
    catch (...) { return fail(h, CDH_BAD_ARG, "unknown C++ exception"); }
}
template <typename F> int32_t guarded(F&& body) { return guarded_as(nullptr, body); }
template <typename F> int32_t guarded(cdh_handle h, F&& body) {
    if (!h) return fail(nullptr, CDH_BAD_ARG, "handle is NULL");
    return guarded_as(h, body);
}

}  // namespace

// ====================================================================================
extern "C" {

int32_t cdh_device_count(int32_t* out) { return guarded([&]() -> int32_t {
    NEED_P(nullptr, out);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_create_error = hipGetErrorString(e); *out = 0; return CDH_HIP_ERROR; }
    *out = n;
    return CDH_OK;
}); }

const char* cdh_last_error(cdh_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int32_t cdh_create(cdh_handle* out, int32_t dtype, int32_t loss, int64_t n_local, int64_t n_total,
                   int64_t row_offset, int64_t p, int32_t device) {
    cdh_handle h = nullptr;           // while it is being built: freed below unless it was handed over
    const int32_t status = guarded([&]() -> int32_t {
    if (!out) return fail(nullptr, CDH_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (dtype != CDH_F64 && dtype != CDH_F32) return fail(nullptr, CDH_BAD_ARG, "dtype must be CDH_F64 or CDH_F32");
    if (loss != CDH_LS && loss != CDH_SQRT && loss != CDH_WLS) return fail(nullptr, CDH_BAD_ARG, "unknown loss");
    if (n_local <= 0 || p <= 0 || n_total < n_local || row_offset < 0 || row_offset + n_local > n_total)
        return fail(nullptr, CDH_DIM_MISMATCH, "need 0 < n_local <= n_total, p > 0, shard inside [0, n_total)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, CDH_HIP_ERROR, "no HIP device: this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, CDH_BAD_ARG, "device index out of range");
    h = new cdh_handle_s();
    h->dtype = dtype; h->loss = loss; h->device = device;
    h->n = n_local; h->n_total = n_total; h->row0 = row_offset; h->p = p;
    h->esz = dtype == CDH_F64 ? 8 : 4;
    h->x.resize(p);
    h->rs.resize(p);
    int32_t rc = [&]() -> int32_t {
        HIPCHK(h, hipSetDevice(device));
        HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        HIPCHK(h, hipEventCreate(&h->prof.ev0));
        HIPCHK(h, hipEventCreate(&h->prof.ev1));
        hipDeviceProp_t prop;
        HIPCHK(h, hipGetDeviceProperties(&prop, device));
        // the padded column, the vectors over it, the chunk's capacity, the default sweep width, the fixed grids, the partials
        h->sz = sweep_sizes(dtype == CDH_F64, n_local, p, std::max(1, prop.multiProcessorCount));
        h->ld = h->sz.ld; h->nvec = h->sz.nvec; h->cap = h->sz.cap; h->blockB = h->sz.blockB;
        h->knobs = read_knobs();
        h->gc.mode = h->knobs.gradient_cache;
        h->gc.cov = h->knobs.gc_cov;
        h->cs.enabled = h->knobs.cov_solve;
        h->cs.helpers = h->knobs.cs_crew;
        h->small.enabled = h->knobs.small_path;
        const size_t colbytes = (size_t)h->ld * h->esz;
        HIPCHK(h, h->X.alloc(colbytes * (size_t)p));
        HIPCHK(h, h->y.alloc(colbytes));
        HIPCHK(h, h->r.alloc(colbytes));
        HIPCHK(h, hipMemsetAsync(h->y, 0, colbytes, h->stream));
        HIPCHK(h, hipMemsetAsync(h->r, 0, colbytes, h->stream));
        if (loss == CDH_WLS) {
            HIPCHK(h, h->w.alloc(colbytes));
            HIPCHK(h, hipMemsetAsync(h->w, 0, colbytes, h->stream));
        }
        HIPCHK(h, h->beta.alloc(sizeof(double) * p));
        HIPCHK(h, hipMemsetAsync(h->beta, 0, sizeof(double) * p, h->stream));
        HIPCHK(h, h->omega.alloc(sizeof(double) * p));
        HIPCHK(h, h->d_ctrl.alloc(sizeof(Ctrl)));
        HIPCHK(h, h->d_idx.alloc(sizeof(int64_t) * h->cap));
        HIPCHK(h, h->d_hs.alloc(sizeof(double) * h->cap));
        HIPCHK(h, h->d_newval.alloc(sizeof(double) * h->cap));
        HIPCHK(h, h->d_touched.alloc(sizeof(int32_t) * h->cap));
        static_assert((size_t)kColBatch * kColChunks * 2 >= (size_t)kGlmMaxGrid * kGlmPoisVals, "the widest IRLS record fits the partials");
        HIPCHK(h, h->d_partials.alloc(sizeof(double) * h->sz.partials_doubles));
        HIPCHK(h, h->d_red.alloc(sizeof(double) * 4096));
        HIPCHK(h, h->d_colout.alloc(sizeof(double) * 2 * p));
        HIPCHK(h, h->d_sup_idx.alloc(sizeof(int64_t) * p));
        HIPCHK(h, h->d_sup_val.alloc(sizeof(double) * p));
        HIPCHK(h, h->h_idx.alloc(sizeof(int64_t) * h->cap));
        HIPCHK(h, h->h_hs.alloc(sizeof(double) * h->cap));
        HIPCHK(h, h->h_newval.alloc(sizeof(double) * h->cap));
        HIPCHK(h, h->h_touched.alloc(sizeof(int32_t) * h->cap));
        HIPCHK(h, h->h_red.alloc(sizeof(double) * 64));
        HIPCHK(h, h->h_ctrl.alloc(sizeof(Ctrl)));
        // zero the pad rows of X once (uploads / the generator only write rows < n)
        if (h->ld > h->n) HIPCHK(h, hipMemsetAsync(h->X, 0, colbytes * (size_t)p, h->stream));
        h->ctrl.lambda0 = 0.0; h->ctrl.n_total = (double)n_total; h->ctrl.maxH = 0.0;
        h->ctrl.loss = loss; h->ctrl.has_omega = 0; h->ctrl.domain_error = 0;
        CHK(upload_ctrl(h));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return CDH_OK;
    }();
    if (rc != CDH_OK) { g_create_error = h->err; return rc; }
    *out = h;
    return CDH_OK;
    });
    if (status != CDH_OK) free_all(h);   // (after a throw as well; nothing to free if it never came to be)
    return status;
}

int32_t cdh_destroy(cdh_handle h) { return guarded([&]() -> int32_t {
    if (!h) return CDH_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    free_all(h);
    return CDH_OK;
}); }

int32_t cdh_synchronize(cdh_handle h) { return guarded(h, [&]() -> int32_t {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}); }

// X or W is about to change (cdh_set_X_cols, cdh_set_obs_weights, cdh_vc_set_data, cdh_vc_set_point): nothing derived from
// them survives -- the carried residual's consistency, the stashed dots, the gradient cache with its Gram columns, the
// one-launch solve's Gram matrix.  With `columns`, r first catches up with what it owes in terms of the OLD columns.
static void small_invalidate(cdh_handle h) { h->small.G_valid = false; h->small.c_valid = false; h->small.rent_paid = 0.0; }
static int32_t design_changes(cdh_handle h, bool columns) {
    if (columns && h->rs.owes_catchup()) {
        HIPCHK(h, hipSetDevice(h->device));
        CHK(sync_r(h));
    }
    h->rs.design_or_loss_changed();
    gc_invalidate(h, true);
    small_invalidate(h);
    return CDH_OK;
}

int32_t cdh_set_X_cols(cdh_handle h, int64_t j0, int64_t ncols, const void* host, int64_t ld) { return guarded(h, [&]() -> int32_t {
    if (ncols > 0) NEED_P(h, host);
    CHK(design_changes(h, true));
    if (j0 < 0 || ncols < 0 || j0 + ncols > h->p || ld < h->n) return fail(h, CDH_DIM_MISMATCH, "column block outside X");
    if (ncols == 0) return CDH_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy2DAsync((char*)h->X + (size_t)j0 * h->ld * h->esz, (size_t)h->ld * h->esz, host,
                               (size_t)ld * h->esz, (size_t)h->n * h->esz, (size_t)ncols,
                               hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}); }

int32_t cdh_get_X_cols(cdh_handle h, int64_t j0, int64_t ncols, void* host, int64_t ld) { return guarded(h, [&]() -> int32_t {
    if (ncols > 0) NEED_P(h, host);
    if (j0 < 0 || ncols < 0 || j0 + ncols > h->p || ld < h->n) return fail(h, CDH_DIM_MISMATCH, "column block outside X");
    if (ncols == 0) return CDH_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy2DAsync(host, (size_t)ld * h->esz, (char*)h->X + (size_t)j0 * h->ld * h->esz,
                               (size_t)h->ld * h->esz, (size_t)h->n * h->esz, (size_t)ncols,
                               hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}); }

int32_t cdh_set_y(cdh_handle h, const void* host_y) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, host_y);
    h->rs.overwritten_with_y();        // r = copy(y) below
    gc_invalidate(h, false);
    h->gc.st.yy_void();
    h->small.c_valid = false;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->y, host_y, (size_t)h->n * h->esz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->r, h->y, (size_t)h->n * h->esz, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->y_set = true;
    return CDH_OK;
}); }

int32_t cdh_get_y(cdh_handle h, void* host_y) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, host_y);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(host_y, h->y, (size_t)h->n * h->esz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}); }

static int32_t ensure_weights_buffer(cdh_handle h) {
    if (h->w) return CDH_OK;
    const size_t colbytes = (size_t)h->ld * h->esz;
    DevBuf<void> w;
    HIPCHK(h, w.alloc(colbytes));
    HIPCHK(h, hipMemsetAsync(w, 0, colbytes, h->stream));
    h->w = std::move(w);
    return CDH_OK;
}

int32_t cdh_set_obs_weights(cdh_handle h, const void* host_w) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, host_w);
    CHK(design_changes(h, false));
    if (h->loss != CDH_WLS) return fail(h, CDH_BAD_ARG, "observation weights need the CDH_WLS loss");
    HIPCHK(h, hipSetDevice(h->device));
    CHK(ensure_weights_buffer(h));
    HIPCHK(h, hipMemcpyAsync(h->w, host_w, (size_t)h->n * h->esz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->has_w = true;
    return CDH_OK;
}); }

int32_t cdh_get_obs_weights(cdh_handle h, void* host_w) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, host_w);
    if (h->loss != CDH_WLS || !h->has_w) return fail(h, CDH_BAD_ARG, "no observation weights are set");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(host_w, h->w, (size_t)h->n * h->esz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}); }

int32_t cdh_set_loss(cdh_handle h, int32_t loss) { return guarded(h, [&]() -> int32_t {
    if (loss != CDH_LS && loss != CDH_SQRT && loss != CDH_WLS) return fail(h, CDH_BAD_ARG, "unknown loss");
    if (loss == h->loss) return CDH_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (loss == CDH_WLS) CHK(ensure_weights_buffer(h));
    h->loss = loss;
    h->ctrl.loss = loss;          // goes to the device with the next chunk's control block
    if (h->has_w) { small_invalidate(h); gc_invalidate(h, true); }   // X'WX is not X'X
    h->has_w = false;             // a weighted loss gets its weights from cdh_set_obs_weights
    h->rs.design_or_loss_changed();
    gc_invalidate(h, false);
    h->domain_error = false;
    return CDH_OK;
}); }

int32_t cdh_generate(cdh_handle h, uint64_t seed, int64_t s, double noise, double* out_beta_star) { return guarded(h, [&]() -> int32_t {
    if (s < 0 || s > h->p) return fail(h, CDH_BAD_ARG, "need 0 <= s <= p");
    h->rs.regenerated();
    gc_invalidate(h, true);
    h->gc.st.yy_void();
    small_invalidate(h);
    HIPCHK(h, hipSetDevice(h->device));
    // The handle starts over as a new one does, down to the memory of the Gram store.  The cache's gates ask whether there is
    // a store (gc_fetch, gc_pass_device, cov_solve), not whether it holds anything: with the old X's store left over, the
    // device loop served the first full pass on the new X where a new handle's host pass does -- the same path of solves
    // with the same counts, and iterates a bit or two apart in the last place (tests/test_gpu_generator.py, LAB_NOTES.md)
    { DevBuf<double> gone = std::move(h->gc.d_G); h->gc.d_G_retired.clear(); h->gc.dev_slots_cap = 0; }
    // planted coefficients: beta*_j = z_j (1 + u_j) (benchmark/cd_bench.jl:14), stream 2
    std::vector<double> bstar((size_t)std::max<int64_t>(s, 1), 0.0);
    for (int64_t j = 0; j < s; ++j) {
        double u1, u2;
        const double z = Philox::normal(seed, (uint64_t)(2 * j), 0u, 2u);
        Philox::uniforms(seed, (uint64_t)j, 1u, 2u, u1, u2);
        bstar[(size_t)j] = z * (1.0 + u1);
    }
    if (out_beta_star) std::memcpy(out_beta_star, bstar.data(), sizeof(double) * (size_t)s);
    HIPCHK(h, hipMemcpyAsync(h->d_sup_val, bstar.data(), sizeof(double) * bstar.size(), hipMemcpyHostToDevice, h->stream));
    const int64_t pairs = (h->n + 3) / 2;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (pairs + kBlock - 1) / kBlock));
    for (int64_t j0 = 0; j0 < h->p; j0 += 32768) {
        const int64_t nc = std::min<int64_t>(32768, h->p - j0);
        CHK(dispatch(h, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            hipLaunchKernelGGL(k_gen_X<T>, dim3(gx, (unsigned)nc), dim3(kBlock), 0, h->stream, (T*)h->X,
                               h->ld, h->n, h->row0, j0, seed);
            return CDH_OK;
        }));
    }
    const int gy = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (h->n + kBlock - 1) / kBlock));
    CHK(dispatch(h, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        hipLaunchKernelGGL(k_gen_y<T>, dim3(gy), dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld, h->n,
                           h->row0, s, h->d_sup_val, noise, seed, (T*)h->y, (T*)h->r);
        return CDH_OK;
    }));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->y_set = true;
    h->x.clear();
    HIPCHK(h, hipMemsetAsync(h->beta, 0, sizeof(double) * h->p, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}); }

int32_t cdh_set_penalty(cdh_handle h, double lambda0, const double* omega, int64_t n_omega) { return guarded(h, [&]() -> int32_t {
    HIPCHK(h, hipSetDevice(h->device));
    bool uploaded = false;
    if (omega) {
        if (n_omega != h->p) return fail(h, CDH_DIM_MISMATCH, "length(g.lambda) != numCoordinates(f)");
        // a path hands over the same weights at every lambda (lasso.jl:251: ProxL1(lambda, stdX)): what the device holds is kept
        if (!(h->omega_dev_ok && (int64_t)h->h_omega.size() == h->p && std::memcmp(h->h_omega.data(), omega, sizeof(double) * (size_t)h->p) == 0)) {
            HIPCHK(h, hipMemcpyAsync(h->omega, omega, sizeof(double) * h->p, hipMemcpyHostToDevice, h->stream));
            h->h_omega.assign(omega, omega + h->p);
            h->omega_dev_ok = true;
            uploaded = true;
        }
        h->has_omega = true;
    } else {
        h->has_omega = false;
    }
    h->ctrl.lambda0 = lambda0;
    h->ctrl.has_omega = h->has_omega ? 1 : 0;
    // the control block goes to the device at the start of every chunk (run_chunk); only the caller's
    // weight buffer, borrowed for this call, has to be consumed before returning
    if (uploaded) HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}); }

int32_t cdh_num_coordinates(cdh_handle h, int64_t* out) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out);
    *out = h->p;
    return CDH_OK;
}); }

static int32_t load_iterate(cdh_handle h, int64_t x_length, int64_t nnz, const int64_t* idx1, const double* val) {
    if (x_length != h->p) return fail(h, CDH_DIM_MISMATCH, "numCoordinates(x) != numCoordinates(f)");
    if (nnz < 0 || nnz > h->p) return fail(h, CDH_BAD_ARG, "nnz out of range");
    if (nnz > 0) { NEED_P(h, idx1); NEED_P(h, val); }
    for (int64_t i = 0; i < nnz; ++i)
        if (idx1[i] < 1 || idx1[i] > h->p) return fail(h, CDH_BAD_ARG, "support index out of range");
    HIPCHK(h, hipSetDevice(h->device));
    h->rs.iterate_loaded();
    h->x.clear();
    for (int64_t i = 0; i < nnz; ++i) {
        // a stored zero keeps its slot in the reference's SparseIterate; mirror that
        if (val[i] == 0.0) { h->x.set(idx1[i] - 1, 1.0); h->x.set(idx1[i] - 1, 0.0); }
        else h->x.set(idx1[i] - 1, val[i]);
    }
    return upload_beta(h, h->x);     // (beta = 0: nothing to upload, nothing to wait for)
}

int32_t cdh_set_iterate(cdh_handle h, int64_t x_length, int64_t nnz, const int64_t* idx1, const double* val) { return guarded(h, [&]() -> int32_t {
    return load_iterate(h, x_length, nnz, idx1, val);
}); }

int32_t cdh_initialize(cdh_handle h, int64_t x_length, int64_t nnz, const int64_t* idx1, const double* val) { return guarded(h, [&]() -> int32_t {
    CHK(load_iterate(h, x_length, nnz, idx1, val));
    return rebuild_residual(h);
}); }

int32_t cdh_descend(cdh_handle h, int64_t k1, double* out_h) { return guarded(h, [&]() -> int32_t {
    return descend(h, k1, out_h);
}); }

int32_t cdh_lambda_max(cdh_handle h, double* out) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out);
    HIPCHK(h, hipSetDevice(h->device));
    return lambda_max(h, out);
}); }

int32_t cdh_pass(cdh_handle h, int64_t m, const int64_t* idx1, double* out_maxH) { return guarded(h, [&]() -> int32_t {
    return pass(h, m, idx1, out_maxH);
}); }

int32_t cdh_solve(cdh_handle h, const cdh_options* opt, cdh_stats* out) { return guarded(h, [&]() -> int32_t {
    return solve_once(h, opt, out);
}); }

int32_t cdh_coordinate_descent(cdh_handle h, const cdh_options* opt, cdh_stats* out) { return guarded(h, [&]() -> int32_t {
    return coordinate_descent(h, opt, out);
}); }

int32_t cdh_get_beta(cdh_handle h, double* out_p) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out_p);
    std::memset(out_p, 0, sizeof(double) * (size_t)h->p);
    for (int64_t s = 0; s < h->x.nnz(); ++s) out_p[h->x.coord(s)] = h->x.slot_value(s);
    return CDH_OK;
}); }

int32_t cdh_get_support(cdh_handle h, int64_t* out_idx1, int64_t* out_nnz) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out_idx1);
    NEED_P(h, out_nnz);
    for (int64_t s = 0; s < h->x.nnz(); ++s) out_idx1[s] = h->x.coord(s) + 1;
    *out_nnz = h->x.nnz();
    return CDH_OK;
}); }

int32_t cdh_get_residual(cdh_handle h, void* out_n_local) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out_n_local);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(sync_r(h));
    HIPCHK(h, hipMemcpyAsync(out_n_local, h->r, (size_t)h->n * h->esz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}); }

// ---- l1-penalised GLMs by IRLS (glm_kernels.hpp; no reference counterpart: a round's solve is the weighted lasso of
// CDWeightedLSLoss, cd_differentiable_function.jl:118-194) ---------------------------------------------------------------------
// The body of cdh_glm_irls, cdh_glm_irls_fold, cdh_glm_poisson_irls and cdh_glm_cox_irls: stands in for cdh_get_residual, w and z on the host,
// cdh_set_y, cdh_set_obs_weights and cdh_initialize between two rounds.  F: the family (GlmBinomial, GlmBinomialFold, GlmPoisson,
// GlmBinomialFoldW and GlmPoissonW where the handle holds observation weights -- chosen by the exports, on the host --
// and GlmCox of cox_kernels.hpp, whose glm_check and glm_launch are its own).
extern "C++" template <class F>
static int32_t glm_step(cdh_handle h, int32_t k, int32_t apply, const GlmParams& pm, double* out) {
    CHK(glm_check<F>(h, k, apply, pm, out));
    HIPCHK(h, hipSetDevice(h->device));
    CHK(glm_catch_up(h));
    if (!apply) return glm_launch<F>(h, k, false, pm, out);      // read-only from here
    // what cdh_set_obs_weights and cdh_set_y void, through their own calls: the residual's consistency and the stashed dots,
    // the gradient cache with its Gram columns, y'y, the one-launch solve's G and c
    CHK(design_changes(h, false));
    gc_invalidate(h, false);
    h->gc.st.yy_void();
    h->small.c_valid = false;
    CHK(ensure_weights_buffer(h));
    CHK(glm_launch<F>(h, k, true, pm, out));
    // r = d / w IS z - X beta of the iterate, but not the bits initialize! would write: consistent, not pristine
    h->rs.rewritten_as_residual();
    gc_after_rebuild(h, h->x);           // (as after cdh_initialize: the cache's reference iterate is the handle's)
    h->has_w = true;
    return CDH_OK;
}

// stands in for cdh_set_y of n zeros, the labels kept beside it
int32_t cdh_glm_set_labels(cdh_handle h, int32_t family, const void* host_labels) { return guarded(h, [&]() -> int32_t {
    return glm_set_labels(h, family, host_labels);
}); }

int32_t cdh_glm_get_labels(cdh_handle h, void* host_labels) { return guarded(h, [&]() -> int32_t {
    return glm_get_labels(h, host_labels);
}); }

// the step between two rounds (glm_step), the binomial family
int32_t cdh_glm_irls(cdh_handle h, int32_t apply, double wmin, double* out3) { return guarded(h, [&]() -> int32_t {
    const GlmParams pm{wmin, 0.0};
    if (!h->glm.weighted) return glm_step<GlmBinomial>(h, -1, apply, pm, out3);
    // with weights: the fold-aware weighted step at k = -1, behind this export's own refusals; the first three sums are its record
    CHK(glm_check<GlmBinomial>(h, -1, apply, pm, out3));
    double out5[kGlmFoldVals];
    CHK(glm_step<GlmBinomialFoldW>(h, -1, apply, pm, out5));
    std::copy(out5, out5 + kGlmVals, out3);
    return CDH_OK;
}); }

// the same step inside a fold of a cross-validated path (cv_path.hpp; the solves are LassoPath's, lasso.jl:229-260, on the
// weighted loss): held-out rows keep weight zero through every round, and their deviance and class error come out of the pass
int32_t cdh_glm_irls_fold(cdh_handle h, int32_t k, int32_t apply, double wmin, double* out5) { return guarded(h, [&]() -> int32_t {
    if (h->glm.weighted) return glm_step<GlmBinomialFoldW>(h, k, apply, GlmParams{wmin, 0.0}, out5);
    return glm_step<GlmBinomialFold>(h, k, apply, GlmParams{wmin, 0.0}, out5);
}); }

// the Poisson family of the same loop: stands in for cdh_set_y of n zeros, the counts and the offset kept beside it
int32_t cdh_glm_set_counts(cdh_handle h, const void* host_counts, const void* host_offset) { return guarded(h, [&]() -> int32_t {
    return glm_set_observations(h, GlmData::Poisson, host_counts, host_offset);
}); }

int32_t cdh_glm_get_offset(cdh_handle h, void* host_offset) { return guarded(h, [&]() -> int32_t {
    return glm_get_offset(h, host_offset);
}); }

int32_t cdh_glm_poisson_irls(cdh_handle h, int32_t k, int32_t apply, double wmin, double eta_max, double* out6) { return guarded(h, [&]() -> int32_t {
    if (h->glm.weighted) return glm_step<GlmPoissonW>(h, k, apply, GlmParams{wmin, eta_max}, out6);
    return glm_step<GlmPoisson>(h, k, apply, GlmParams{wmin, eta_max}, out6);
}); }

// observation weights of the binomial and the Poisson family: stands in for the v in cdh_set_obs_weights of v w, composed on
// the host every round
int32_t cdh_glm_set_weights(cdh_handle h, const void* host_weights) { return guarded(h, [&]() -> int32_t {
    return glm_set_weights(h, host_weights, [&]() -> int32_t { return design_changes(h, false); });
}); }

int32_t cdh_glm_get_weights(cdh_handle h, void* host_weights) { return guarded(h, [&]() -> int32_t {
    return glm_get_weights(h, host_weights);
}); }

// the Cox family of the same loop (cox_kernels.hpp): stands in for cdh_set_y of n zeros, the times sorted on the host, the
// status and the offset kept where the other families keep their observations
int32_t cdh_glm_set_survival(cdh_handle h, const void* host_time, const void* host_status, const void* host_offset) { return guarded(h, [&]() -> int32_t {
    return cox_set_survival(h, host_time, host_status, host_offset);
}); }

int32_t cdh_glm_get_survival(cdh_handle h, void* host_time, void* host_status) { return guarded(h, [&]() -> int32_t {
    return cox_get_survival(h, host_time, host_status);
}); }

// the same with strata (segments of the order, at which the scans restart) and observation weights; both NULL: the call above
int32_t cdh_glm_set_survival_strata(cdh_handle h, const void* host_time, const void* host_status, const void* host_offset, const int32_t* host_strata, const void* host_weights) { return guarded(h, [&]() -> int32_t {
    return cox_set_survival(h, host_time, host_status, host_offset, host_strata, host_weights);
}); }

int32_t cdh_glm_set_survival_interval(cdh_handle h, const void* host_start, const void* host_stop, const void* host_status, const void* host_offset, const int32_t* host_strata, const void* host_weights) { return guarded(h, [&]() -> int32_t {
    return cox_set_survival(h, host_stop, host_status, host_offset, host_strata, host_weights, host_start);
}); }

int32_t cdh_glm_get_survival_start(cdh_handle h, void* host_start) { return guarded(h, [&]() -> int32_t {
    return cox_get_survival_start(h, host_start);
}); }

int32_t cdh_glm_get_survival_strata(cdh_handle h, int32_t* host_strata, void* host_weights) { return guarded(h, [&]() -> int32_t {
    return cox_get_survival_strata(h, host_strata, host_weights);
}); }

int32_t cdh_glm_cox_irls(cdh_handle h, int32_t k, int32_t apply, double wmin, double eta_max, double* out5) { return guarded(h, [&]() -> int32_t {
    return glm_step<GlmCox>(h, k, apply, GlmParams{wmin, eta_max}, out5);
}); }

int32_t cdh_glm_set_cox_ties(cdh_handle h, int32_t ties) { return guarded(h, [&]() -> int32_t {
    return cox_set_ties(h, ties);
}); }

int32_t cdh_glm_get_cox_ties(cdh_handle h, int32_t* ties) { return guarded(h, [&]() -> int32_t {
    return cox_get_ties(h, ties);
}); }

// what survival work is done with, at the iterate the handle holds (cox_post_host.hpp, cox_post.hip)
int32_t cdh_glm_cox_residuals(cdh_handle h, double eta_max, void* host_cumhaz_or_null, void* host_martingale_or_null, void* host_deviance_or_null) { return guarded(h, [&]() -> int32_t {
    return cox_post_residuals(h, eta_max, host_cumhaz_or_null, host_martingale_or_null, host_deviance_or_null);
}); }

int32_t cdh_glm_cox_baseline(cdh_handle h, double eta_max, int64_t capacity, int32_t* host_stratum, void* host_time, void* host_n_event, void* host_risk_sum, void* host_cumhaz, void* host_cumvar, int64_t* count) { return guarded(h, [&]() -> int32_t {
    return cox_post_baseline(h, eta_max, capacity, host_stratum, host_time, host_n_event, host_risk_sum, host_cumhaz, host_cumvar, count);
}); }

// what a survival model is judged by: the concordance index of the held-out rows, or of all (cox_concordance_host.hpp)
int32_t cdh_glm_cox_concordance(cdh_handle h, int32_t k, double* out4) { return guarded(h, [&]() -> int32_t {
    return cox_concordance(h, k, out4);
}); }

// what inference after a Cox fit is made of: score and Schoenfeld residuals, the information matrix (cox_score_host.hpp, cox_score.hip)
int32_t cdh_glm_cox_score(cdh_handle h, double eta_max, int64_t m, const int64_t* idx1, const double* host_centre_or_null, double* host_centre_out_or_null, void* host_schoenfeld_or_null, void* host_score_or_null, double* host_info_or_null) { return guarded(h, [&]() -> int32_t {
    return cox_score(h, eta_max, m, idx1, host_centre_or_null, host_centre_out_or_null, host_schoenfeld_or_null, host_score_or_null, host_info_or_null);
}); }

// ---- cross-validation of a lasso path (cv_path.hpp; the solves are lasso.jl:229-260 on 0/1 weights, utils.jl:140-151) ------
int32_t cdh_set_folds(cdh_handle h, const int32_t* fold_of_row, int32_t K, int64_t* out_count) { return guarded(h, [&]() -> int32_t {
    return cv_set_folds(h, fold_of_row, K, out_count);
}); }

// leaves the handle as cdh_set_obs_weights with the same values would
int32_t cdh_set_fold_weights(cdh_handle h, int32_t k) { return guarded(h, [&]() -> int32_t {
    CHK(cv_check_fold_weights(h, k));
    CHK(design_changes(h, false));
    HIPCHK(h, hipSetDevice(h->device));
    CHK(ensure_weights_buffer(h));
    CHK(cv_write_fold_weights(h, k));
    h->has_w = true;
    return CDH_OK;
}); }

int32_t cdh_path_sse(cdh_handle h, int32_t k, int64_t s, const int64_t* idx1, int64_t m, const double* B, int64_t ldb,
                     double* out_held, double* out_train) { return guarded(h, [&]() -> int32_t {
    return cv_path_sse(h, k, s, idx1, m, B, ldb, out_held, out_train);
}); }

// ---- varying-coefficient mode (vc_host.hpp; varying_coefficient_lasso.jl:30-79) ----------------------------------------------
}  // extern "C"
namespace {
#include "vc_host.hpp"   // vc_set_data, vc_point; the scratch, the launch body and the group planners of cdh_vc_gram and cdh_vc_gram_batch
}  // namespace
extern "C" {

int32_t cdh_vc_set_data(cdh_handle h, int64_t p_base, int32_t degree, const void* host_X, int64_t ld,
                                    const void* host_z) { return guarded(h, [&]() -> int32_t {
    return vc_set_data(h, p_base, degree, host_X, ld, host_z);
}); }

int32_t cdh_vc_set_point(cdh_handle h, int32_t kernel_kind, double bandwidth, double z0, double* out_std) { return guarded(h, [&]() -> int32_t {
    return vc_point(h, kernel_kind, bandwidth, z0, -1, out_std, nullptr);
}); }

// :109-113 and the scores of _findLargestCorrelations(w, X, y, s) (utils.jl:108-124) for the point z0 = z[row0], row0 left out
int32_t cdh_vc_set_point_loo(cdh_handle h, int32_t kernel_kind, double bandwidth, int64_t row0, double* out_std,
                             double* out_scores) { return guarded(h, [&]() -> int32_t {
    if (row0 < 0 || row0 >= h->n) return fail(h, CDH_BAD_ARG, "the left-out row is outside 0 .. n - 1");
    if (!h->y_set) return fail(h, CDH_BAD_ARG, "the screening scores need y: cdh_set_y first");
    return vc_point(h, kernel_kind, bandwidth, 0.0, row0, out_std, out_scores);
}); }

int32_t cdh_vc_gram(cdh_handle h, int32_t kernel_kind, double bandwidth, double z0, int64_t leave_out_row0, int32_t wpow,
                    const void* host_e, int64_t mb, const int64_t* base_idx1, double* out_G, double* out_c,
                    double* out_sum_w) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out_G);
    NEED_P(h, base_idx1);
    CHK(vc_refuse_shards(h));
    if (const char* bad = vc_gram_check(h->vc_degree, h->y_set, out_c != nullptr, h->vc_pbase, h->n, kernel_kind, bandwidth, z0,
                                        leave_out_row0, wpow, mb, base_idx1))
        return fail(h, CDH_BAD_ARG, bad);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(vc_gram_scratch(h));
    VcGramScratch& g = h->vg;
    if (vc_gram_grid(h->n, h->vc_degree, mb) * vc_gram_rec(h->vc_degree, mb).n > kVgPartialDoubles)
        return fail(h, CDH_BAD_ARG, "cdh_vc_gram: partial buffer too small for this grid");
    return vc_gram_run(h, kernel_kind, 1, &bandwidth, &z0, &leave_out_row0, wpow, host_e, mb, base_idx1, out_G, out_c, out_sum_w,
                       VcGramBufs{g.partials, g.out, g.h_out, &g.in->pt, &g.h_in->pt}, false, 1, vc_gram_one_group);
}); }

int32_t cdh_vc_gram_batch(cdh_handle h, int32_t kernel_kind, int64_t m, const double* bandwidth, const double* z0,
                          const int64_t* leave_out_row0, int32_t wpow, const void* host_e, int64_t mb,
                          const int64_t* base_idx1, double* out_G, double* out_c, double* out_sum_w) { return guarded(h, [&]() -> int32_t {
    if (!out_G) return fail(h, CDH_BAD_ARG, "cdh_vc_gram_batch: out_G is NULL");
    CHK(vc_refuse_shards(h));
    int64_t bad_point = -1;
    if (const char* bad = vc_gram_batch_check(h->vc_degree, h->y_set, out_c != nullptr, h->vc_pbase, h->n, kernel_kind, m,
                                              bandwidth, z0, leave_out_row0, wpow, mb, base_idx1, &bad_point)) {
        char buf[256];
        if (bad_point < 0) return fail(h, CDH_BAD_ARG, bad);
        snprintf(buf, sizeof buf, "cdh_vc_gram_batch: point %lld: %s", (long long)bad_point, bad);
        return fail(h, CDH_BAD_ARG, buf);
    }
    // every point has passed; nothing has been launched or allocated before this line
    HIPCHK(h, hipSetDevice(h->device));
    CHK(vc_gram_scratch(h));
    CHK(vc_gram_batch_scratch(h));
    VcGramBatchScratch& b = h->vgb;
    return vc_gram_run(h, kernel_kind, m, bandwidth, z0, leave_out_row0, wpow, host_e, mb, base_idx1, out_G, out_c, out_sum_w,
                       VcGramBufs{b.partials, b.out, b.h_out, b.pts, b.h_pts}, vgb_resident(h->n, h->vc_degree, mb),
                       vgb_groups(h->n, h->vc_degree, mb, m), vc_gram_batch_group);
}); }

// ---- the read-only statistics (col_stats.hpp) -------------------------------------------------------------------------------------
}  // extern "C"
namespace {
#include "col_stats.hpp"   // the bodies of the exports below; gram_launch, gram_block; lambda_max
}  // namespace
extern "C" {

int32_t cdh_gradient(cdh_handle h, int64_t k1, double* out) { return guarded(h, [&]() -> int32_t {
    return gradient(h, k1, out);
}); }

int32_t cdh_col_rms(cdh_handle h, double* out_p) { return guarded(h, [&]() -> int32_t {
    return col_rms(h, out_p);
}); }

int32_t cdh_col_wrms(cdh_handle h, double* out_p) { return guarded(h, [&]() -> int32_t {
    return col_wrms(h, out_p);
}); }

int32_t cdh_loadings(cdh_handle h, double* out_p) { return guarded(h, [&]() -> int32_t {
    return loadings(h, out_p);
}); }

int32_t cdh_xt_r(cdh_handle h, double* out_p) { return guarded(h, [&]() -> int32_t {
    return xt_r(h, out_p);
}); }

int32_t cdh_xt_r_cols(cdh_handle h, int64_t m, const int64_t* idx1, double* out_m) { return guarded(h, [&]() -> int32_t {
    return xt_r_cols(h, m, idx1, out_m);
}); }

int32_t cdh_gram(cdh_handle h, int64_t m, const int64_t* idx1, double* out_G, double* out_c, double* out_q) { return guarded(h, [&]() -> int32_t {
    return gram_block(h, m, idx1, out_G, out_c, out_q, false);
}); }

int32_t cdh_gram_weighted(cdh_handle h, int64_t m, const int64_t* idx1, double* out_G, double* out_c, double* out_q) { return guarded(h, [&]() -> int32_t {
    return gram_weighted(h, m, idx1, out_G, out_c, out_q);
}); }

int32_t cdh_get_X_row(cdh_handle h, int64_t row0, int64_t m, const int64_t* idx1, double* out_m) { return guarded(h, [&]() -> int32_t {
    return get_X_row(h, row0, m, idx1, out_m);
}); }

int32_t cdh_resid_moments(cdh_handle h, double* out_sum, double* out_sumsq) { return guarded(h, [&]() -> int32_t {
    return resid_moments(h, out_sum, out_sumsq);
}); }

int32_t cdh_resid_wmoments(cdh_handle h, double* out_sum_w, double* out_sum_wr2) { return guarded(h, [&]() -> int32_t {
    return resid_wmoments(h, out_sum_w, out_sum_wr2);
}); }

int32_t cdh_resid_std(cdh_handle h, double* out_std, double* out_mean) { return guarded(h, [&]() -> int32_t {
    return resid_std(h, out_std, out_mean);
}); }

int32_t cdh_objective(cdh_handle h, double* out) { return guarded(h, [&]() -> int32_t {
    return objective(h, out);
}); }

int32_t cdh_set_reuse_residual(cdh_handle h, int32_t on) { return guarded(h, [&]() -> int32_t {
    h->reuse_residual = on != 0;
    return CDH_OK;
}); }

int32_t cdh_set_sweep_mode(cdh_handle h, int32_t mode, int32_t block) { return guarded(h, [&]() -> int32_t {
    if (mode != CDH_SWEEP_COORD && mode != CDH_SWEEP_BLOCK) return fail(h, CDH_BAD_ARG, "unknown sweep mode");
    if (mode == CDH_SWEEP_BLOCK && block != 2 && block != 4 && block != 8 && block != 16 && block != 32 && block != 64)
        return fail(h, CDH_BAD_ARG, "block size must be 2, 4, 8, 16, 32 or 64");
    h->mode = mode;
    if (mode == CDH_SWEEP_BLOCK) { h->blockB = block; h->width_default = false; }   // the caller's choice: the caller keeps the ranks alike
    return CDH_OK;
}); }

int32_t cdh_set_screening(cdh_handle h, int32_t on) { return guarded(h, [&]() -> int32_t {
    if (on < 0 || on > 2) return fail(h, CDH_BAD_ARG, "screening: 0 = never, 1 = solves, 2 = cdh_pass as well");
    h->screening = on;
    return CDH_OK;
}); }

int32_t cdh_set_gradient_cache(cdh_handle h, int32_t mode) { return guarded(h, [&]() -> int32_t {
    if (mode < 0 || mode > 3) return fail(h, CDH_BAD_ARG, "gradient cache: 0 = off, 1 = rent-or-buy, 2 = from the first full pass, 3 = 2 without the size guard");
    if (mode == 0) gc_invalidate(h, true);
    h->gc.mode = mode;
    h->gc.cooldown = 0; h->gc.backoff = 1;
    return CDH_OK;
}); }

int32_t cdh_set_onchip_solve(cdh_handle h, int32_t on) { return guarded(h, [&]() -> int32_t {
    h->small.enabled = on != 0;
    return CDH_OK;
}); }

int32_t cdh_onchip_stats(cdh_handle h, int64_t* out2) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out2);
    out2[0] = h->small.n_solves; out2[1] = h->small.n_gram;
    return CDH_OK;
}); }

int32_t cdh_onchip_last(cdh_handle h, int64_t* out3) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out3);
    out3[0] = out3[1] = out3[2] = 0;
    if (h->small.h_ctl) { out3[0] = h->small.h_ctl->steps; out3[1] = (int64_t)h->small.h_ctl->cycles; out3[2] = (int64_t)h->small.h_ctl->ticks; }
    return CDH_OK;
}); }

int32_t cdh_get_gradient_cache(cdh_handle h, int32_t* out_mode) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out_mode);
    *out_mode = h->gc.mode;
    return CDH_OK;
}); }

int32_t cdh_cache_drift(cdh_handle h, int32_t rereference_now, double* out3) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out3);
    GradCache& c = h->gc;
    if (rereference_now && c.st.valid() && gc_applicable(h)) {
        HIPCHK(h, hipSetDevice(h->device));
        CHK(gc_rereference(h));
    }
    out3[0] = c.drift_last; out3[1] = c.drift_max; out3[2] = (double)c.n_drift;
    return CDH_OK;
}); }

int32_t cdh_cache_stats(cdh_handle h, int64_t* out10) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out10);
    const GradCache& c = h->gc;
    out10[0] = c.n_passes; out10[1] = c.n_certified; out10[2] = c.n_exact;
    out10[3] = c.n_validate; out10[4] = c.n_batches; out10[5] = c.n_columns;
    out10[6] = c.n_cov; out10[7] = c.n_reconcile; out10[8] = c.n_rollbacks;
    out10[9] = c.n_dev_passes;
    return CDH_OK;
}); }

int32_t cdh_cache_gram_column(cdh_handle h, int64_t k1, double* out_p, double* out_eps) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out_p);
    CHK(check_coordinate(h, k1));
    GradCache& c = h->gc;
    if (c.slot.empty() || c.slot[(size_t)(k1 - 1)] < 0 || (size_t)c.slot[(size_t)(k1 - 1)] >= c.G.size())
        return fail(h, CDH_BAD_ARG, "the gradient cache holds no Gram column for this coordinate");
    HIPCHK(h, hipSetDevice(h->device));
    CHK(gc_host_column(h, c.slot[(size_t)(k1 - 1)]));
    const std::vector<double>& col = c.G[(size_t)c.slot[(size_t)(k1 - 1)]];
    std::memcpy(out_p, col.data(), sizeof(double) * (size_t)h->p);
    if (out_eps) *out_eps = h->dtype == CDH_F32 ? 5.9604644775390625e-8 * kCrossF32EpsFactor / std::sqrt((double)h->n_total) : 0.0;
    return CDH_OK;
}); }

int32_t cdh_set_device_loop(cdh_handle h, int32_t on) { return guarded(h, [&]() -> int32_t {
    h->cs.enabled = on != 0;
    if (on == 2) h->cs.helpers = 0;                 // the loop without its helper workgroups
    else if (on > 2) h->cs.helpers = std::min(kCsCrewMax, on);
    return CDH_OK;
}); }

int32_t cdh_device_loop_stats(cdh_handle h, int64_t* out12) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out12);
    out12[0] = h->cs.n_launches; out12[1] = h->cs.n_passes; out12[2] = h->cs.n_folds; out12[3] = h->cs.n_exact;
    for (int i = 0; i < 8; ++i) out12[4 + i] = h->cs.ticks[i];
    return CDH_OK;
}); }

int32_t cdh_device_loop_table(cdh_handle h, int64_t* out6 /* eight values by now */) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out6);
    out6[0] = h->cs.n_table_passes; out6[1] = h->cs.n_table_rows; out6[2] = h->gc.st.table_entries(); out6[3] = kCsTableCap;
    out6[4] = h->gc.n_forced_rounds; out6[5] = h->cs.n_forced_rounds; out6[6] = h->cs.n_crew_passes; out6[7] = h->cs.n_crew_jobs;
    return CDH_OK;
}); }

int32_t cdh_set_use_graph(cdh_handle h, int32_t on) { return guarded(h, [&]() -> int32_t {
    h->use_graph = on != 0;
    if (on) h->graph_broken = false;   // asking again retries a capture that failed earlier
    return CDH_OK;
}); }

int32_t cdh_comm_unique_id(void* out_128_bytes) { return guarded([&]() -> int32_t {
    NEED_P(nullptr, out_128_bytes);
    std::string err;
    if (!load_rccl(err)) { g_create_error = err; return CDH_RCCL_ERROR; }
    UniqueId id;
    std::memset(&id, 0, sizeof id);
    if (g_rccl.GetUniqueId(&id) != 0) { g_create_error = "ncclGetUniqueId failed"; return CDH_RCCL_ERROR; }
    std::memcpy(out_128_bytes, &id, sizeof id);
    return CDH_OK;
}); }

int32_t cdh_comm_init(cdh_handle h, const void* id_128_bytes, int32_t rank, int32_t nranks) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, id_128_bytes);
    CHK(refused(h, h->xs.comm_refused(rank, nranks)));
    // a 1-rank communicator is only built when asked for (exercises the RCCL path on one GPU)
    if (nranks == 1 && !h->knobs.force_rccl) { h->xs.comm_not_needed(); return CDH_OK; }
    std::string err;
    if (!load_rccl(err)) { h->err = err; return CDH_RCCL_ERROR; }
    HIPCHK(h, hipSetDevice(h->device));
    UniqueId id;
    std::memcpy(&id, id_128_bytes, sizeof id);
    void* comm = nullptr;
    int rc = ((comm_init_rank_fn)g_rccl.CommInitRank)(&comm, nranks, id, rank);
    if (rc != 0) {
        h->err = std::string("ncclCommInitRank failed: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
        return CDH_RCCL_ERROR;
    }
    h->xs.comm_installed(comm, rank, nranks);   // an exchange is installed (again, after a cdh_comm_drop)
    return CDH_OK;
}); }

int32_t cdh_comm_drop(cdh_handle h) { return guarded(h, [&]() -> int32_t {
    void* comm = h->xs.communicator();
    if (!comm) return CDH_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->graphs.clear();   // captured passes hold the communicator's all-reduces
    if (g_rccl.CommAbort) g_rccl.CommAbort(comm); else if (g_rccl.CommDestroy) g_rccl.CommDestroy(comm);
    h->xs.comm_dropped();
    return CDH_OK;
}); }

// ---- optional direct exchange (p2p_exchange.hpp) -------------------------------------------------
int32_t cdh_p2p_local_handle(cdh_handle h, void* out_64_bytes) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, out_64_bytes);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size is part of the ABI");
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->p2p_inbox) {
        DevBuf<unsigned long long> inbox; DevBuf<unsigned> base; PinBuf<int> timeout;
        // polled by this GPU while peers write it: must not be served from a stale L2 line
        if (inbox.alloc(kP2PInboxBytes, hipDeviceMallocUncached) != hipSuccess)
            HIPCHK(h, inbox.alloc(kP2PInboxBytes, hipDeviceMallocFinegrained));
        HIPCHK(h, hipMemset(inbox, 0, kP2PInboxBytes));  // tag 0 = never written; epochs start at 1
        HIPCHK(h, base.alloc(sizeof(unsigned)));
        HIPCHK(h, hipMemset(base, 0, sizeof(unsigned)));
        HIPCHK(h, timeout.alloc(sizeof(int)));
        *timeout = 0;
        HIPCHK(h, hipDeviceSynchronize());
        h->p2p_inbox = std::move(inbox); h->d_p2p_base = std::move(base); h->p2p_timeout = std::move(timeout);
    }
    hipIpcMemHandle_t ipc;
    HIPCHK(h, hipIpcGetMemHandle(&ipc, h->p2p_inbox));
    std::memcpy(out_64_bytes, &ipc, sizeof ipc);
    return CDH_OK;
}); }

int32_t cdh_p2p_connect(cdh_handle h, const void* handles_64_bytes_each, int32_t rank, int32_t nranks) { return guarded(h, [&]() -> int32_t {
    NEED_P(h, handles_64_bytes_each);
    CHK(refused(h, h->xs.p2p_connect_refused(rank, nranks, h->p2p_inbox != nullptr)));
    HIPCHK(h, hipSetDevice(h->device));
    for (int q = 0; q < nranks; ++q) {
        if (q == rank) { h->p2p_peers.inbox[q] = h->p2p_inbox; continue; }
        hipIpcMemHandle_t ipc;
        std::memcpy(&ipc, (const char*)handles_64_bytes_each + 64 * (size_t)q, sizeof ipc);
        void* mapped = nullptr;
        HIPCHK(h, hipIpcOpenMemHandle(&mapped, ipc, hipIpcMemLazyEnablePeerAccess));
        h->p2p_mapped.push_back(mapped);
        h->p2p_peers.inbox[q] = (unsigned long long*)mapped;
    }
    h->xs.p2p_connected(rank, nranks);
    return CDH_OK;
}); }

int32_t cdh_p2p_enable(cdh_handle h, int32_t on) { return guarded(h, [&]() -> int32_t {
    if (!on) { h->xs.p2p_disabled(); return CDH_OK; }
    return refused(h, h->xs.p2p_enabled(h->xs.direct_ranks() && *(volatile int*)h->p2p_timeout));   // (connected: the flag is there)
}); }

int32_t cdh_set_host_exchange(cdh_handle h, cdh_host_allreduce_fn fn, void* user, int32_t rank, int32_t nranks) { return guarded(h, [&]() -> int32_t {
    if (!fn) { h->xs.host_removed(); return CDH_OK; }
    CHK(refused(h, h->xs.host_refused(rank, nranks)));
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->h_xchg) {   // the longest record is the 2p column dots of _findLambdaMax / _stdX!
        const size_t doubles = (size_t)std::max<int64_t>(4096, 2 * h->p);
        HIPCHK(h, h->h_xchg.alloc(sizeof(double) * doubles));
        h->h_xchg_doubles = doubles;
    }
    h->xs.host_installed(fn, user, rank, nranks);
    return CDH_OK;
}); }

int32_t cdh_exchange_stats(cdh_handle h, int64_t* out_rccl_calls, int64_t* out_p2p_calls, int64_t* out_host_calls,
                           int32_t* out_nranks) { return guarded(h, [&]() -> int32_t {
    const cdh::ExchangeState& xs = h->xs;
    if (out_rccl_calls) *out_rccl_calls = xs.rccl_calls();
    if (out_p2p_calls) *out_p2p_calls = xs.direct_calls();
    if (out_host_calls) *out_host_calls = xs.host_calls();
    if (out_nranks) {
        int n = xs.reported_ranks();
        // with a communicator: what the communicator itself says, not what we asked for
        if (xs.communicator() && g_rccl.CommCount && g_rccl.CommCount(xs.communicator(), &n) != 0) n = -1;
        *out_nranks = n;
    }
    return CDH_OK;
}); }

int32_t cdh_exchange_probe(cdh_handle h, double* inout, int64_t count) { return guarded(h, [&]() -> int32_t {
    if (count < 0 || count > 4096 || (count > 0 && !inout)) return fail(h, CDH_BAD_ARG, "probe: 0 <= count <= 4096");
    if (!h->d_red) return fail(h, CDH_BAD_ARG, "probe: handle has no data yet");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->d_red, inout, sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
    CHK(allreduce(h, h->d_red, (size_t)count));
    HIPCHK(h, hipMemcpyAsync(inout, h->d_red, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return p2p_check(h);
}); }

int32_t cdh_exchange_latency(cdh_handle h, int64_t count, int32_t iters, double* out_us) { return guarded(h, [&]() -> int32_t {
    if (count < 1 || count > 4096 || iters < 1 || iters > 100000 || !out_us) return fail(h, CDH_BAD_ARG, "latency probe: 1 <= count <= 4096, 1 <= iters <= 100000");
    if (!h->d_red) return fail(h, CDH_BAD_ARG, "probe: handle has no data yet");
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->prof.ev0) { HIPCHK(h, hipEventCreate(&h->prof.ev0)); HIPCHK(h, hipEventCreate(&h->prof.ev1)); }
    HIPCHK(h, hipMemsetAsync(h->d_red, 0, sizeof(double) * (size_t)count, h->stream));
    for (int i = 0; i < 3; ++i) CHK(allreduce(h, h->d_red, (size_t)count));   // warm the path
    HIPCHK(h, hipEventRecord(h->prof.ev0, h->stream));
    for (int i = 0; i < iters; ++i) CHK(allreduce(h, h->d_red, (size_t)count));
    HIPCHK(h, hipEventRecord(h->prof.ev1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    CHK(p2p_check(h));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->prof.ev0, h->prof.ev1));
    *out_us = (double)ms * 1e3 / iters;
    return CDH_OK;
}); }

int32_t cdh_profile_begin(cdh_handle h) { return guarded(h, [&]() -> int32_t {
    h->prof.on = true; h->prof.ms = 0.0; h->prof.bytes = 0.0; h->prof.launches = 0;
    return CDH_OK;
}); }

int32_t cdh_profile_end(cdh_handle h, double* out_ms, int64_t* out_launches, double* out_algorithmic_bytes) { return guarded(h, [&]() -> int32_t {
    h->prof.on = false;
    if (out_ms) *out_ms = h->prof.ms;
    if (out_launches) *out_launches = h->prof.launches;
    if (out_algorithmic_bytes) *out_algorithmic_bytes = h->prof.bytes;
    return CDH_OK;
}); }

// ---- cdh_quad: CDQuadraticLoss, a batch of problems on one A (quad_solve.hpp) -------------------------------------------------
int32_t cdh_quad_create(cdh_quad* out, int64_t p, int64_t max_batch, int32_t device) { return guarded([&]() -> int32_t {
    QNEED(out, "out is NULL");
    *out = nullptr;
    QREFUSE(quad_check_create(p, max_batch));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return quad_fail(CDH_HIP_ERROR, "no HIP device: this library has no CPU fallback");
    QNEED(device >= 0 && device < ndev, "device index out of range");
    QuadOwner own{new cdh_quad_s()};       // freed on every early return below
    cdh_quad q = own.q;
    q->p = p; q->max_batch = max_batch; q->device = device;
    q->lds_bytes = (unsigned)quad_lds_bytes(p);
    QCHK(hipSetDevice(device));
    QCHK(hipStreamCreateWithFlags(&q->stream, hipStreamNonBlocking));
    CHK(quad_alloc(q));
    // a problem's state may take more dynamic LDS than a kernel gets unasked (64 KiB): up to the CU's 160 KiB
    if (q->lds_bytes > 48 * 1024) {
        QCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_quad_solve<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQuadLdsBudget));
        QCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_quad_solve<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQuadLdsBudget));
    }
    *out = own.release();
    return CDH_OK;
}); }

int32_t cdh_quad_destroy(cdh_quad q) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    quad_free(q);
    return CDH_OK;
}); }

int32_t cdh_quad_set_A(cdh_quad q, const double* A, int64_t lda) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QNEED(A, "A is NULL");
    QNEED(lda >= q->p, "lda must be at least p");
    QCHK(hipSetDevice(q->device));
    const size_t p = (size_t)q->p;
    std::vector<double> inv(p);
    for (size_t k = 0; k < p; ++k) {
        const double d = A[k + (size_t)lda * k];
        QNEED(d > 0.0, "diag(A) must be positive");
        inv[k] = 1.0 / d;                  // a = 1 / A_kk (cd_differentiable_function.jl:326), once per A
    }
    QCHK(hipMemcpy2DAsync(q->A, sizeof(double) * p, A, sizeof(double) * (size_t)lda, sizeof(double) * p, p, hipMemcpyHostToDevice, q->stream));
    QCHK(hipMemcpyAsync(q->inv_a, inv.data(), sizeof(double) * p, hipMemcpyHostToDevice, q->stream));
    QCHK(hipStreamSynchronize(q->stream));
    q->A_set = true;
    return CDH_OK;
}); }

int32_t cdh_quad_set_b(cdh_quad q, int64_t m, const double* B, int64_t ldb) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QNEED(B, "B is NULL");
    QNEED(m >= 1, "m must be positive");
    if (m > q->max_batch) {
        char buf[160];
        snprintf(buf, sizeof buf, "m = %lld problems exceed the handle's max_batch = %lld", (long long)m, (long long)q->max_batch);
        return quad_fail(CDH_BAD_ARG, buf);
    }
    QNEED(ldb >= q->p, "ldb must be at least p");
    QCHK(hipSetDevice(q->device));
    const size_t p = (size_t)q->p;
    q->h_B.resize(p * (size_t)m);
    for (int64_t j = 0; j < m; ++j) std::memcpy(q->h_B.data() + (size_t)j * p, B + (size_t)j * (size_t)ldb, sizeof(double) * p);
    q->m = m; q->penalty_set = false; q->host_stale = true;
    QCHK(hipMemcpyAsync(q->B, q->h_B.data(), sizeof(double) * p * (size_t)m, hipMemcpyHostToDevice, q->stream));
    QCHK(hipMemcpyAsync(q->g, q->h_B.data(), sizeof(double) * p * (size_t)m, hipMemcpyHostToDevice, q->stream));   // Ax = 0 (:304-308)
    QCHK(hipMemsetAsync(q->beta, 0, sizeof(double) * p * (size_t)m, q->stream));
    QCHK(hipMemsetAsync(q->nnz, 0, sizeof(int32_t) * (size_t)m, q->stream));
    QCHK(hipStreamSynchronize(q->stream));
    return CDH_OK;
}); }

int32_t cdh_quad_set_penalty(cdh_quad q, const double* lambda0, const double* omega, int64_t ldo) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QNEED(lambda0, "lambda0 is NULL");
    QNEED(q->m > 0, "no problems are loaded: cdh_quad_set_b first");
    QNEED(!omega || ldo == 0 || ldo >= q->p, "ldo must be 0 (one shared vector) or at least p");
    QCHK(hipSetDevice(q->device));
    const size_t p = (size_t)q->p, m = (size_t)q->m;
    q->h_lambda0.assign(lambda0, lambda0 + m);
    q->has_omega = omega != nullptr; q->omega_shared = omega && ldo == 0;
    const size_t ncol = !omega ? 0 : (ldo == 0 ? 1 : m);
    q->h_omega.resize(p * ncol);
    for (size_t j = 0; j < ncol; ++j) std::memcpy(q->h_omega.data() + j * p, omega + j * (size_t)ldo, sizeof(double) * p);
    QCHK(hipMemcpyAsync(q->lambda0, q->h_lambda0.data(), sizeof(double) * m, hipMemcpyHostToDevice, q->stream));
    if (ncol) QCHK(hipMemcpyAsync(q->omega, q->h_omega.data(), sizeof(double) * p * ncol, hipMemcpyHostToDevice, q->stream));
    QCHK(hipStreamSynchronize(q->stream));
    q->penalty_set = true;
    return CDH_OK;
}); }

int32_t cdh_quad_set_iterate(cdh_quad q, int64_t j, int64_t nnz, const int64_t* idx1, const double* val) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QREFUSE(quad_check_problem(j, q->m));
    QNEED(nnz == 0 || (idx1 && val), "idx1 or val is NULL");
    std::vector<unsigned char> seen((size_t)q->p, 0);
    QREFUSE(quad_check_support(q->p, nnz, idx1, seen.data()));
    QCHK(hipSetDevice(q->device));
    const size_t p = (size_t)q->p;
    std::vector<double> dense(p, 0.0);
    std::vector<int32_t> sup((size_t)nnz);
    for (int64_t s = 0; s < nnz; ++s) { sup[(size_t)s] = (int32_t)(idx1[s] - 1); dense[(size_t)(idx1[s] - 1)] = val[s]; }
    const int32_t n32 = (int32_t)nnz;
    QCHK(hipMemcpyAsync(q->beta + (size_t)j * p, dense.data(), sizeof(double) * p, hipMemcpyHostToDevice, q->stream));
    if (nnz) QCHK(hipMemcpyAsync(q->sup + (size_t)j * p, sup.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, q->stream));
    QCHK(hipMemcpyAsync(q->nnz + j, &n32, sizeof(int32_t), hipMemcpyHostToDevice, q->stream));
    QCHK(hipStreamSynchronize(q->stream));
    q->host_stale = true;
    return CDH_OK;
}); }

int32_t cdh_quad_get_iterate(cdh_quad q, int64_t j, int64_t* nnz, int64_t* idx1, double* val) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QREFUSE(quad_check_problem(j, q->m));
    QNEED(nnz && idx1 && val, "nnz, idx1 or val is NULL");
    QCHK(hipSetDevice(q->device));
    CHK(quad_pull(q));
    const size_t p = (size_t)q->p, off = (size_t)j * p;
    const int32_t n = q->h_nnz[(size_t)j];
    for (int32_t s = 0; s < n; ++s) { const int32_t k = q->h_sup[off + (size_t)s]; idx1[s] = (int64_t)k + 1; val[s] = q->h_beta[off + (size_t)k]; }
    *nnz = n;
    return CDH_OK;
}); }

int32_t cdh_quad_initialize(cdh_quad q) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    CHK(quad_ready(q, false));
    hipLaunchKernelGGL(k_quad_init, dim3((unsigned)q->m), dim3(256), 0, q->stream, (int)q->p, q->A, q->B, q->beta, q->sup, q->nnz, q->g);
    QCHK(hipGetLastError());
    QCHK(hipStreamSynchronize(q->stream));
    return CDH_OK;
}); }

int32_t cdh_quad_get_gradient(cdh_quad q, int64_t j, double* out) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QREFUSE(quad_check_problem(j, q->m));
    QNEED(out, "out is NULL");
    QCHK(hipSetDevice(q->device));
    QCHK(hipMemcpyAsync(out, q->g + (size_t)j * (size_t)q->p, sizeof(double) * (size_t)q->p, hipMemcpyDeviceToHost, q->stream));
    QCHK(hipStreamSynchronize(q->stream));
    return CDH_OK;
}); }

int32_t cdh_quad_descend(cdh_quad q, int64_t j, int64_t k1, double* out_h) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QNEED(out_h, "out_h is NULL");
    return quad_explicit(q, j, 1, &k1, false, nullptr, out_h);
}); }

int32_t cdh_quad_pass(cdh_quad q, int64_t j, int64_t n, const int64_t* idx1, double* maxH) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QNEED(maxH, "maxH is NULL");
    return quad_explicit(q, j, n, idx1, true, maxH, nullptr);
}); }

int32_t cdh_quad_coordinate_descent(cdh_quad q, const cdh_options* opt, cdh_stats* stats) { return guarded([&]() -> int32_t {
    QNEED(q, "quad handle is NULL");
    QNEED(opt, "opt is NULL");
    return quad_coordinate_descent(q, opt, stats);
}); }

}  // extern "C"

// the start-stop chain of the Cox step, LAST: its kernels are emitted behind every other kernel (the reason is in the file)
namespace {
#include "cox_interval.hpp"
#include "cox_efron_host.hpp"   // the Efron chain's host body: no kernel of its own (they are cox_efron.hip's, the second unit)
}  // namespace
