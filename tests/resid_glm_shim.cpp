// Test-only C shim over csrc/resid_state.hpp for the transition cdh_glm_irls(apply = 1) added (rewritten_as_residual), compiled
// with g++ and driven on the CPU by tests/test_glm_host.py.  tests/resid_shim.cpp stays as it is; this file repeats the few
// entry points the new test needs, in the order cdhip.hip calls the transitions.
#include <cstdint>
#include <vector>
#include "../coordinatedescent.jl_amd/csrc/resid_state.hpp"

using cdh::ResidState;
using cdh::SupportList;

namespace {
struct State { int64_t p; ResidState rs; };
SupportList iterate(int64_t p, int64_t nnz, const int64_t* idx, const double* val) {
    SupportList x(p);
    for (int64_t i = 0; i < nnz; ++i) x.set(idx[i], val[i]);
    return x;
}
}  // namespace

extern "C" {
void* rg_new(int64_t p) { auto* s = new State(); s->p = p; s->rs.resize(p); return s; }
void rg_free(void* s) { delete (State*)s; }
#define RS (((State*)s)->rs)
// rebuild_residual_from: 1 if skipped as a no-op
int rg_rebuild(void* s, int64_t nnz, const int64_t* idx, const double* val) {
    const SupportList x = iterate(((State*)s)->p, nnz, idx, val);
    if (RS.rebuild_is_noop(x)) { RS.rebuild_skipped(); return 1; }
    RS.rebuild_begins();
    RS.rebuilt_from(x);
    return 0;
}
// cdh_glm_irls(apply = 1) after its catch-up: design_changes, then the kernel, then the new transition
void rg_irls_apply(void* s) { RS.design_or_loss_changed(); RS.rewritten_as_residual(); }
void rg_rewritten(void* s) { RS.rewritten_as_residual(); }
void rg_set_y(void* s) { RS.overwritten_with_y(); }
void rg_stream(void* s, int64_t launches) { RS.stream_begins(); RS.stream_enqueued(launches); }
void rg_moved(void* s, int64_t k, double d) { RS.moved(k, d); }
void rg_left_lazy(void* s, int64_t nnz, const int64_t* idx, const double* val) { RS.left_lazy(iterate(((State*)s)->p, nnz, idx, val)); }
void rg_dots_taken(void* s, int64_t len, int weighted) { RS.dots_taken(std::vector<double>((size_t)len, 1.0), weighted != 0); }
int rg_consistent(void* s) { return RS.consistent(); }
int rg_lazy(void* s) { return RS.lazy(); }
int rg_owes(void* s) { return RS.owes_catchup(); }
int64_t rg_roundings(void* s) { return RS.roundings(); }
int64_t rg_skipped(void* s) { return RS.rebuilds_skipped(); }
int rg_noop(void* s, int64_t nnz, const int64_t* idx, const double* val) { return RS.rebuild_is_noop(iterate(((State*)s)->p, nnz, idx, val)); }
int rg_can_adopt(void* s, int weighted, int64_t p) { return RS.can_adopt_dots(weighted != 0, p); }
}
