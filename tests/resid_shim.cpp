// Test-only C shim over csrc/resid_state.hpp (the move ledger and the residual's state), compiled with g++
// and driven on the CPU by tests/test_resid_state.py.  rs_rebuild and rs_demand call the transitions in the
// order rebuild_residual_from and sync_r (csrc/cdhip.hip) call them; everything else is one method each.
#include <cstdint>
#include <vector>
#include "../coordinatedescent.jl_amd/csrc/resid_state.hpp"

using cdh::MoveLedger;
using cdh::ResidState;
using cdh::SupportList;

namespace {
struct State { int64_t p; ResidState rs; };
SupportList iterate(int64_t p, int64_t nnz, const int64_t* idx, const double* val) {
    SupportList x(p);
    for (int64_t i = 0; i < nnz; ++i) x.set(idx[i], val[i]);
    return x;
}
int rebuild(ResidState& rs, const SupportList& x) {     // rebuild_residual_from: 1 if skipped
    if (rs.rebuild_is_noop(x)) { rs.rebuild_skipped(); return 1; }
    rs.rebuild_begins();
    rs.rebuilt_from(x);
    return 0;
}
}  // namespace

extern "C" {
void* ml_new(int64_t p) { auto* m = new MoveLedger(); m->resize(p); return m; }
void ml_free(void* m) { delete (MoveLedger*)m; }
void ml_add(void* m, int64_t k, double d) { ((MoveLedger*)m)->add(k, d); }
void ml_set(void* m, int64_t k, double v) { ((MoveLedger*)m)->set(k, v); }
void ml_clear(void* m) { ((MoveLedger*)m)->clear(); }
double ml_value(void* m, int64_t k) { return ((MoveLedger*)m)->value(k); }
int ml_contains(void* m, int64_t k) { return ((MoveLedger*)m)->contains(k); }
int ml_empty(void* m) { return ((MoveLedger*)m)->empty(); }
int64_t ml_size(void* m) { return (int64_t)((MoveLedger*)m)->size(); }
void ml_members(void* m, int64_t* out, int64_t* out_by_index) {     // by iteration, and through operator[]
    auto& L = *(MoveLedger*)m;
    int64_t i = 0;
    for (int64_t k : L) out[i++] = k;
    for (size_t j = 0; j < L.size(); ++j) out_by_index[j] = L[j];
}

void* rs_new(int64_t p) { auto* s = new State(); s->p = p; s->rs.resize(p); return s; }
void rs_free(void* s) { delete (State*)s; }
#define RS (((State*)s)->rs)
// transitions
void rs_stream(void* s, int64_t launches) { RS.stream_begins(); RS.stream_enqueued(launches); }
int rs_rebuild(void* s, int64_t nnz, const int64_t* idx, const double* val) { return rebuild(RS, iterate(((State*)s)->p, nnz, idx, val)); }
// sync_r: 2 a lazy residual formed, 3 ... and found in the buffer already; else the batches of 64 the catch-up applied
int rs_demand(void* s) {
    if (RS.lazy()) { const SupportList x = RS.take_lazy(); return 2 + rebuild(RS, x); }
    if (RS.pending().empty()) return 0;
    RS.catchup_begins();
    int batches = 0;
    for (size_t o = 0; o < RS.pending().size(); o += 64) { RS.catchup_batch_applied(); ++batches; }
    RS.catchup_done();
    return -batches;
}
void rs_set_y(void* s) { RS.overwritten_with_y(); }
void rs_generate(void* s) { RS.regenerated(); }
void rs_design_or_loss(void* s) { RS.design_or_loss_changed(); }
void rs_iterate_loaded(void* s) { RS.iterate_loaded(); }
void rs_iterate_moved(void* s) { RS.iterate_moved(); }
void rs_moved(void* s, int64_t k, double d) { RS.moved(k, d); }
void rs_left_lazy(void* s, int64_t nnz, const int64_t* idx, const double* val) { RS.left_lazy(iterate(((State*)s)->p, nnz, idx, val)); }
void rs_dots_taken(void* s, const double* cd, int64_t len, int weighted) { RS.dots_taken(std::vector<double>(cd, cd + len), weighted != 0); }
int64_t rs_adopt(void* s, double* out) {
    const std::vector<double>& cd = RS.adopt_dots();
    for (size_t i = 0; i < cd.size(); ++i) out[i] = cd[i];
    return (int64_t)cd.size();
}
// what readers ask
int rs_consistent(void* s) { return RS.consistent(); }
int rs_lazy(void* s) { return RS.lazy(); }
int rs_owes(void* s) { return RS.owes_catchup(); }
int64_t rs_roundings(void* s) { return RS.roundings(); }
int64_t rs_skipped(void* s) { return RS.rebuilds_skipped(); }
int64_t rs_adopted(void* s) { return RS.dots_adopted(); }
int rs_noop(void* s, int64_t nnz, const int64_t* idx, const double* val) { return RS.rebuild_is_noop(iterate(((State*)s)->p, nnz, idx, val)); }
int rs_can_adopt(void* s, int weighted, int64_t p) { return RS.can_adopt_dots(weighted != 0, p); }
int64_t rs_pending(void* s, int64_t* out_k, double* out_v) {
    int64_t i = 0;
    for (int64_t k : RS.pending()) { out_k[i] = k; out_v[i] = RS.pending().value(k); ++i; }
    return i;
}
}
