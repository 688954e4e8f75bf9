// ctypes surface of csrc/solve_plan.hpp for tests/test_solve_plan_host.py: one function per rule, results as flat arrays.
#include <string.h>

#include "../coordinatedescent.jl_amd/csrc/solve_plan.hpp"

extern "C" {

int64_t so_c_const(const char* name) {
#define K(x) if (!strcmp(name, #x)) return (int64_t)(x)
    K(kScreen); K(kScreenMax); K(kScreenMinPass); K(kNoSupportLimit);
#undef K
    return -1;
}
int so_c_grid(double lmax, double target, int64_t numSteps, double* out) { return cold_start_grid(lmax, target, numSteps, out) ? 1 : 0; }
double so_c_lambda_max(const double* v, int64_t stride, int64_t p, double denom, const double* omega) {
    return lambda_max_of(v, stride, p, denom, omega);
}
// The walk over m visits with mover[i] telling whether a screen stops at visit i.  out: (kind, pos, len, hit) per step, kind 1 a
// screen (hit: how many it settled), kind 0 a stream (hit: -1); at most max_steps are written.  Returns the number of steps.
int64_t so_c_walk(int64_t m, int B, int64_t cap, int64_t p, const uint8_t* mover, int64_t* out, int64_t max_steps) {
    ScreenWalk walk(m, B, cap, p);
    int64_t n = 0;
    while (!walk.done()) {
        const ScreenStep s = walk.next();
        int hit = -1;
        if (s.screen) {
            hit = s.len;
            for (int i = 0; i < s.len; ++i) if (mover[s.pos + i]) { hit = i; break; }
            walk.hit(hit);
        }
        if (n < max_steps) { out[4 * n] = s.screen ? 1 : 0; out[4 * n + 1] = s.pos; out[4 * n + 2] = s.len; out[4 * n + 3] = hit; }
        ++n;
    }
    return n;
}
int so_c_weights_ready(int wls, int has_w) { return weights_ready(wls != 0, has_w != 0) ? 1 : 0; }
int so_c_screen_gate(int screening, int wls, int has_w, int64_t m, int64_t nnz, int64_t p) {
    return screen_gate(screening, wls != 0, has_w != 0, m, nnz, p) ? 1 : 0;
}
int64_t so_c_rows_limit(int64_t n_total, int64_t rows_per_nnz, int exempt) { return rows_support_limit(n_total, rows_per_nnz, exempt != 0); }
// out: (prev_converged, converged, iter, finished) after each pass, up to the one that finishes; returns how many
int so_c_progress(const double* maxH, int n, double optTol, int64_t* out) {
    SolveProgress at;
    int k = 0;
    while (k < n) {
        const bool done = at.pass_done(maxH[k], optTol);
        out[4 * k] = at.prev_converged; out[4 * k + 1] = at.converged; out[4 * k + 2] = at.iter; out[4 * k + 3] = done;
        ++k;
        if (done) break;
    }
    return k;
}

}  // extern "C"
