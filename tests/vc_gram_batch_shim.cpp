// C entry points over csrc/vc_gram_batch_types.hpp for tests/test_vc_gram_batch_host.py (ctypes): host-only, no HIP.
#include "../coordinatedescent.jl_amd/csrc/vc_gram_batch_types.hpp"

extern "C" {
int vgb_c_resident(int64_t n, int Q, int64_t mb) { return vgb_resident(n, Q, mb) ? 1 : 0; }
int64_t vgb_c_chunks(int64_t n) { return vc_gram_chunks(n); }
int64_t vgb_c_grid(int64_t n, int Q, int64_t mb) { return vc_gram_grid(n, Q, mb); }
int64_t vgb_c_group_points(int64_t n, int Q, int64_t mb) { return vgb_group_points(n, Q, mb); }
int64_t vgb_c_groups(int64_t n, int Q, int64_t mb, int64_t m) { return vgb_groups(n, Q, mb, m); }
int64_t vgb_c_group_first(int64_t n, int Q, int64_t mb, int64_t g) { return vgb_group_first(n, Q, mb, g); }
int64_t vgb_c_group_size(int64_t n, int Q, int64_t mb, int64_t m, int64_t g) { return vgb_group_size(n, Q, mb, m, g); }
int64_t vgb_c_share_points(int64_t n, int Q, int64_t mb, int64_t pts) { return vgb_share_points(n, Q, mb, pts); }
int64_t vgb_c_grid_y(int64_t n, int Q, int64_t mb, int64_t pts) { return vgb_grid_y(n, Q, mb, pts); }
int64_t vgb_c_share_begin(int64_t n, int Q, int64_t mb, int64_t pts, int64_t s) { return vgb_share_begin(n, Q, mb, pts, s); }
int64_t vgb_c_rec_offset(int64_t n, int Q, int64_t mb, int64_t point, int64_t block) { return vgb_rec_offset(n, Q, mb, point, block); }
int64_t vgb_c_device_bytes() { return vgb_scratch_device_bytes(); }
int64_t vgb_c_pinned_bytes() { return vgb_scratch_pinned_bytes(); }
int64_t vgb_c_point_bytes() { return (int64_t)sizeof(VcGramPoint); }
const char* vgb_c_check(int vc_degree, int y_set, int want_c, int64_t p_base, int64_t n, int32_t kind, int64_t m, const double* h,
                        const double* z0, const int64_t* leave_out, int32_t wpow, int64_t mb, const int64_t* idx1,
                        int64_t* bad_point) {
    return vc_gram_batch_check(vc_degree, y_set != 0, want_c != 0, p_base, n, kind, m, h, z0, leave_out, wpow, mb, idx1, bad_point);
}
}
