// ctypes surface of csrc/stats_plan.hpp for tests/test_stats_plan_host.py: one function per plan, results as flat int64 arrays.
#include <string.h>

#include "../coordinatedescent.jl_amd/csrc/stats_plan.hpp"

extern "C" {

int64_t st_c_const(const char* name) {
#define K(x) if (!strcmp(name, #x)) return (int64_t)(x)
    K(kGramMaxCols); K(kGramGroupCols); K(kGramLaunchCols); K(kGsOffC); K(kGsOffQ); K(kGsRec);
#undef K
    return -1;
}
int st_c_rec_g(int s, int l) { return gs_g(s, l); }
int64_t st_c_gram_launches(int64_t m) { return gram_launches(m); }
// out: the columns of launch t, by position; returns how many
int st_c_gram_launch(int64_t m, int64_t t, int64_t* out) {
    const GramLaunch L = gram_launch_at(m, t);
    for (int pos = 0; pos < L.cols(); ++pos) out[pos] = L.col_of(pos);
    return L.cols();
}
// out: (a0, na, b0, nb) of every launch, in order
void st_c_gram_groups(int64_t m, int64_t* out) {
    for (int64_t t = 0; t < gram_launches(m); ++t) {
        const GramLaunch L = gram_launch_at(m, t);
        out[4 * t] = L.a0; out[4 * t + 1] = L.na; out[4 * t + 2] = L.b0; out[4 * t + 3] = L.nb;
    }
}
void st_c_gram_scatter(int64_t m, int64_t t, const double* rec, double* out_G, double* out_c, double* out_q) {
    gram_scatter(gram_launch_at(m, t), m, rec, out_G, out_c, out_q);
}
int64_t st_c_vc_batches(int64_t p) { return vc_batches(p); }
// out: b0, b1, jb0, jb1, chunks, table, partials
void st_c_vc_batch(int64_t p, int degree, int64_t nvec, int cus, int loo, int64_t t, int64_t* out) {
    const VcBatch B = vc_batch(p, degree, nvec, cus, loo != 0, t);
    const int64_t v[7] = {B.b0, B.b1, B.jb0, B.jb1, B.chunks, (int64_t)B.table, (int64_t)B.partials};
    memcpy(out, v, sizeof v);
}
int64_t st_c_vc_launches(int64_t p, int degree) { return vc_point_launches(p, degree); }
double st_c_vc_bytes(int64_t n, int64_t esz, int64_t p) { return vc_point_bytes(n, (size_t)esz, p); }
int64_t st_c_partials_doubles(int f64, int64_t n, int64_t p, int cus) { return (int64_t)sweep_sizes(f64 != 0, n, p, cus).partials_doubles; }

}  // extern "C"
