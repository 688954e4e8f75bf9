// Test-only C shim over csrc/cache_state.hpp (what the gradient cache knows about its data), compiled with g++ and
// driven on the CPU by tests/test_cache_state.py.  Each function calls the transitions in the order the named host
// function of csrc/ calls them, with the device work left out; cs_snapshot reads every query.
#include <cstdint>
#include <vector>
#include "../coordinatedescent.jl_amd/csrc/cache_state.hpp"

using cdh::CacheState;
using cdh::MoveKind;
using cdh::SupportList;

namespace {
struct State { int64_t p; CacheState st; };
SupportList iterate(int64_t p, int64_t nnz, const int64_t* idx, const double* val) {
    SupportList x(p);
    for (int64_t i = 0; i < nnz; ++i) x.set(idx[i], val[i]);
    return x;
}
}  // namespace

extern "C" {
void* cs_new(int64_t p) { auto* s = new State(); s->p = p; return s; }
void cs_free(void* s) { delete (State*)s; }
#define ST (((State*)s)->st)
#define P (((State*)s)->p)
// gc_size, gc_dev_reserve (first use), gc_invalidate
void cs_size(void* s, int consistent, int64_t nnz, const int64_t* idx, const double* val) { ST.size(P, consistent != 0, iterate(P, nnz, idx, val)); }
void cs_mirrors_allocated(void* s) { ST.mirrors_allocated(); }
void cs_invalidate(void* s, int columns) { ST.invalidated(columns != 0); }
// gc_adopt_dots; gc_rereference around gc_validate (fail: the dots-only pass over X failed)
void cs_adopt(void* s) { const bool known = ST.beta_known(); ST.invalidated(false); ST.referenced(known); }
void cs_rereference(void* s, int fail) { const bool known = ST.beta_known(); ST.invalidated(false); if (!fail) ST.referenced(known); }
// gc_after_rebuild
void cs_rebuilt(void* s, int64_t nnz, const int64_t* idx, const double* val) { ST.rebuilt(iterate(P, nnz, idx, val), P); }
// gc_note_moves: stops at the first move the state has nothing more to hear after
void cs_streamed(void* s, int64_t m, const int64_t* idx, const double* hs) {
    for (int64_t i = 0; i < m; ++i)
        if (hs[i] != 0.0 && !ST.moved(idx[i], hs[i], MoveKind::streamed)) return;
}
// cov_apply_visit (ref_takes_nan 0) and cov_solve's note_move (1)
void cs_carried(void* s, int64_t k, double d, int ref_takes_nan) { if (d != 0.0) ST.moved(k, d, MoveKind::carried, ref_takes_nan != 0); }
// small_solve's tail
void cs_small_solve(void* s, int from_c, int64_t m, const int64_t* idx, const double* d) {
    if (from_c) { if (ST.tracks_r()) ST.invalidated(false); }
    for (int64_t i = 0; i < m && !from_c; ++i) if (d[i] != 0.0) ST.moved(idx[i], d[i], MoveKind::off_stream, false);
    ST.q_void();
}
// gc_need_host_g, gc_need_dev_g
void cs_need_host_g(void* s) { if (!ST.host_g_current()) ST.host_g_fetched(); }
void cs_need_dev_g(void* s) { if (!ST.dev_a_current()) ST.dev_a_uploaded(); if (!ST.dev_g_current()) ST.dev_g_uploaded(); }
void cs_host_g_fetched(void* s) { ST.host_g_fetched(); }
void cs_dev_slot_uploaded(void* s) { ST.dev_slot_uploaded(); }
void cs_dev_g_moved_on(void* s) { ST.dev_g_moved_on(); }
void cs_dev_g_rejected(void* s) { ST.dev_g_rejected(); }
void cs_dev_g_rolled_back(void* s, int host_was_current) { ST.dev_g_rolled_back(host_was_current != 0); }
// gc_fold: 0 the device folds, 1 it could not and the host does, 2 ... and the fetch of g fails, 3 a HIP failure mid-fold
void cs_fold(void* s, int how) {
    if (ST.moved().empty()) return;
    bool on_device = false;
    if (how == 0 || how == 3) {          // gc_fold_device got as far as gc_need_dev_g
        cs_need_dev_g(s);
        if (how == 0) { ST.dev_g_moved_on(); on_device = true; }
        else if (ST.host_g_current()) ST.dev_g_dropped();
        else ST.invalidated(false);
    }
    if (!on_device) {
        if (!ST.valid()) return;
        if (how != 2) cs_need_host_g(s);
        ST.dev_g_dropped();
    }
    ST.folded();
}
void cs_pending_replaced(void* s, int32_t n, const int32_t* idx, const double* val) { ST.pending_replaced(idx, val, n); }
void cs_cov_visited(void* s, int64_t m) { ST.cov_visited(m); }
void cs_yy_summed(void* s, double v) { ST.yy_summed(v); }
void cs_yy_void(void* s) { ST.yy_void(); }
void cs_q_summed(void* s, double v) { ST.q_summed(v); }
void cs_q_carried(void* s, double v) { ST.q_carried(v); }
void cs_q_guard(void* s, double factor) { ST.q_guard(factor); }
void cs_q_void(void* s) { ST.q_void(); }
void cs_table_allocated(void* s) { ST.table_allocated(); }
void cs_table_reset_done(void* s) { ST.table_reset_done(); }
void cs_table_holds(void* s, int32_t n) { ST.table_holds(n); }
void cs_prepared(void* s, int go, double cert_abs) { ST.prepared(go != 0, cert_abs); }
void cs_prepared_no_go(void* s) { ST.prepared_no_go(); }
int cs_take_prepared(void* s, double* cert_abs) { return ST.prepared() ? (ST.take_prepared(cert_abs) ? 1 : 2) : 0; }   // gc_full_pass
void cs_unprepared(void* s) { ST.unprepared(); }
void cs_forced_marks_set(void* s) { ST.forced_marks_set(); }
void cs_forced_guard(void* s) { if (ST.forced_marks_dirty()) ST.forced_marks_wiped(); }                          // ~ForcedGuard
int cs_stalled_twice(void* s, int no_progress) { return ST.stalled_twice(no_progress != 0); }

// every query: 17 numbers, then beta_ref (p), then the ledger (returned: its size; members and values)
int64_t cs_snapshot(void* s, double* out, double* beta_ref, int64_t* mk, double* mv) {
    const CacheState& c = ST;
    const double q[17] = {(double)c.sized(), (double)c.valid(), (double)c.beta_known(), (double)c.tracks_r(), (double)c.cov_since_ref(),
                          (double)c.host_g_current(), (double)c.dev_g_current(), (double)c.dev_a_current(), (double)c.dev_slot_current(),
                          (double)c.yy_current(), c.yy(), (double)c.q_usable(), c.q(), c.q_exact(), (double)c.table_void(),
                          (double)c.table_entries(), (double)c.prepared() + 2.0 * (double)c.forced_marks_dirty()};
    for (int i = 0; i < 17; ++i) out[i] = q[i];
    for (size_t k = 0; k < c.beta_ref().size(); ++k) beta_ref[k] = c.beta_ref()[k];
    int64_t i = 0;
    for (int64_t k : c.moved()) { mk[i] = k; mv[i] = c.moved().value(k); ++i; }
    return i;
}
}
