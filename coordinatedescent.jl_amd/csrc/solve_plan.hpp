// solve_plan.hpp -- the host-only arithmetic every solve goes through (solve.hpp, and the places that share a rule with it): the
// lambda grid of a cold start and the lambda_max it starts from, the walk of a screened full pass, the gates that decide whether
// a full pass is screened and whether a weighted loss is ready, the gradient cache's rows-per-non-zero rule, and where the pass
// loop stands.  No HIP in here: tests/test_solve_plan_host.py compiles it with g++ (tests/solve_plan_main.cpp) and holds it to
// tests/_solve_plan.py.  The driver launches, reads back and replays; nothing else decides these numbers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

// ---- the cold start (coordinate_descent.jl:25-36) ---------------------------------------------------------------------------------
// _findLambdaMax (:118-149) over a strided vector of dots: max_k |v_k / denom| / omega_k.  (`t > lmax`: a NaN never wins.)
inline double lambda_max_of(const double* v, int64_t stride, int64_t p, double denom, const double* omega /* or NULL */) {
    double lmax = 0.0;
    for (int64_t k = 0; k < p; ++k) {
        double t = std::fabs(-v[k * stride] / denom);
        if (omega) t /= omega[k];
        if (t > lmax) lmax = t;
    }
    return lmax;
}
// The numSteps + 1 lambdas of exp.(range(log(lmax), log(target), length = numSteps + 1)) (:32-36): the last one is the target's
// own logarithm, not the accumulated sum.  false, and nothing of `out` to be used: the range has a zero (or NaN) step.
inline bool cold_start_grid(double lmax, double target, int64_t numSteps, double* out) {
    const double l1 = std::log(lmax), l2 = std::log(target);
    const double step = (l2 - l1) / (double)numSteps;
    if (step == 0.0 || step != step) return false;
    for (int64_t j = 0; j <= numSteps; ++j) out[j] = std::exp((j == numSteps) ? l2 : l1 + (double)j * step);
    return true;
}

// ---- the gates ---------------------------------------------------------------------------------------------------------------------
constexpr int kScreenMinPass = 16;   // screens / the cache: passes over fewer coordinates than that are a block or two anyway
// a weighted loss only once its weights are there (they are zero until cdh_set_obs_weights: every a_k would be zero)
constexpr bool weights_ready(bool weighted_loss, bool has_w) { return !weighted_loss || has_w; }
// is a full pass of m visits screened?  (full passes over dense iterates are not screened at all)
constexpr bool screen_gate(int screening, bool weighted_loss, bool has_w, int64_t m, int64_t nnz, int64_t p) {
    return screening && weights_ready(weighted_loss, has_w) && m >= kScreenMinPass && nnz * 4 <= p;
}

// ---- the walk of a screened full pass (screened_full_pass) -------------------------------------------------------------------------
// A screen takes the dots of the next S visits and settles those ahead of the first that can move (`hit`; S: all of them).  After
// a hit the visit that can move streams with its Gram block (max(B, 1) visits), and the next `cool` visits are not screened --
// in stretches of max(cool, B), at most `cap`; `cool` doubles on repeated hits, up to m.  A screen that settles all of its columns
// doubles the next one (64 -> 1024 columns, never more than p or cap: the dots' buffer holds 2 p values) and ends the doubling
// of `cool`.
constexpr int kScreen = 64, kScreenMax = 1024;
struct ScreenStep {
    bool screen;     // take the dots of visits [pos, pos + len) and report the hit -- or stream them
    int64_t pos;
    int len;
};
class ScreenWalk {
    int64_t m_, B_, cap_, scr_max_;
    int64_t pos_ = 0, cool_ = 0, cool_len_ = kScreen, scr_;
    int S_ = 0;
    bool after_hit_ = false;
    ScreenStep stream(int64_t mm) { const ScreenStep s{false, pos_, (int)mm}; pos_ += mm; return s; }
public:
    ScreenWalk(int64_t m, int B, int64_t cap, int64_t p)
        : m_(m), B_(B), cap_(cap), scr_max_(std::min<int64_t>({(int64_t)kScreenMax, p, cap})), scr_(std::min<int64_t>(kScreen, scr_max_)) {}
    static constexpr int longest_screen() { return kScreenMax; }
    bool done() const { return pos_ >= m_; }
    ScreenStep next() {                  // while !done(); after a screen step, hit() comes first
        if (after_hit_) {                // the visit that can move
            after_hit_ = false;
            cool_ = cool_len_; cool_len_ = std::min<int64_t>(cool_len_ * 2, m_);
            scr_ = std::min<int64_t>(kScreen, scr_max_);
            return stream(std::min<int64_t>(std::max<int64_t>(B_, 1), m_ - pos_));
        }
        if (cool_ > 0) {                 // unscreened stretch: whole Gram blocks
            const int64_t mm = std::min<int64_t>({cap_, m_ - pos_, std::max<int64_t>(cool_, B_)});
            cool_ -= mm;
            return stream(mm);
        }
        S_ = (int)std::min<int64_t>(scr_, m_ - pos_);
        return ScreenStep{true, pos_, S_};
    }
    void hit(int hit) {                  // visits [pos, pos + hit) of the screen are settled
        pos_ += hit;
        if (hit < S_) { after_hit_ = true; return; }
        cool_len_ = kScreen;
        scr_ = std::min<int64_t>(scr_ * 2, scr_max_);
    }
};

// ---- the gradient cache's rows-per-non-zero rule -----------------------------------------------------------------------------------
// The largest support the cache pays for on long columns: nnz * rows_per_nnz <= n_total.  `exempt`: no such limit.
constexpr int64_t kNoSupportLimit = INT64_MAX;
constexpr int64_t rows_support_limit(int64_t n_total, int64_t rows_per_nnz, bool exempt) {
    return exempt ? kNoSupportLimit : n_total / rows_per_nnz;
}

// ---- where the pass loop stands (_coordinateDescent!, coordinate_descent.jl:65-92) -------------------------------------------------
struct SolveProgress {
    bool prev_converged = false, converged = true;      // the pass to come is a full one while `converged`
    int64_t iter = 0;
    bool pass_done(double maxH, double optTol) {        // true: two passes in a row below optTol, the solve is over
        prev_converged = converged;
        converged = maxH < optTol;
        ++iter;
        return prev_converged && converged;
    }
};
