// C entry points over csrc/vc_gram_types.hpp for tests/test_vc_gram_host.py (ctypes): host-only, no HIP.
#include "../coordinatedescent.jl_amd/csrc/vc_gram_types.hpp"

extern "C" {
int64_t vg_nrec(int Q, int64_t mb) { return vc_gram_rec(Q, mb).n; }
int64_t vg_tri(int64_t mb, int64_t j, int64_t k) { return vc_gram_tri(mb, j, k); }
int64_t vg_off_m(int Q, int64_t mb) { return vc_gram_rec(Q, mb).off_m; }
int64_t vg_off_w(int Q, int64_t mb) { return vc_gram_rec(Q, mb).off_w; }
int vg_pairs(int64_t mb) { return vc_gram_pairs(mb); }
int vg_slices(int64_t mb) { return vc_gram_slices(mb); }
int vg_grid(int64_t n, int Q, int64_t mb) { return vc_gram_grid(n, Q, mb); }
int64_t vg_chain(int64_t n, int Q, int64_t mb) { return vc_gram_chain(n, Q, mb); }
void vg_scatter(int Q, int64_t mb, const double* rec, double* G, double* c) { vc_gram_scatter(Q, mb, rec, G, c); }
const char* vg_check(int vc_degree, int y_set, int want_c, int64_t p_base, int64_t n, int32_t kind, double h, double z0,
                     int64_t leave_out, int32_t wpow, int64_t mb, const int64_t* idx1) {
    return vc_gram_check(vc_degree, y_set != 0, want_c != 0, p_base, n, kind, h, z0, leave_out, wpow, mb, idx1);
}
}
