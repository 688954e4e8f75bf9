// C entry points over csrc/small_plan.hpp for tests/test_small_plan_host.py (ctypes): host-only, no HIP.
#include "../coordinatedescent.jl_amd/csrc/small_plan.hpp"

extern "C" {
int64_t sp_c_state_bytes(int64_t p) { return (int64_t)small_state_bytes(p); }
int sp_c_fits(int64_t p, int64_t budget) { return small_plan(p, (size_t)budget).fits ? 1 : 0; }
int sp_c_ncache(int64_t p, int64_t budget) { return small_plan(p, (size_t)budget).ncache; }
int64_t sp_c_lds_bytes(int64_t p, int64_t budget) { return (int64_t)small_plan(p, (size_t)budget).lds_bytes; }
int sp_c_unroll(int64_t p) { return small_unroll(p); }
int64_t sp_c_ctl_bytes() { return (int64_t)sizeof(SmallCtl); }
int64_t sp_c_sup_off() { return (int64_t)small_sup_off(); }
int64_t sp_c_beta_off(int64_t p) { return (int64_t)small_beta_off(p); }
int64_t sp_c_io_bytes(int64_t p) { return (int64_t)small_io_bytes(p); }
int64_t sp_c_max_p() { return kSmallMaxP; }
int64_t sp_c_max_lam() { return kSmallMaxLam; }
}
