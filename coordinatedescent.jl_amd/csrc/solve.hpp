// solve.hpp -- the driver every solve goes through: a section of cdhip.hip kept in its own file (included once, inside
// cdhip.hip's anonymous namespace, where screened_full_pass stood: behind sweep.hpp, grad_cache.hpp, small_solve.hpp and
// cov_solve.hpp, whose passes it strings together).  A pass (run_pass, screened where a full pass over a sparse iterate pays for
// it), the pass loop (solve), and the bodies of cdh_descend, cdh_pass, cdh_solve and cdh_coordinate_descent.  What it decides
// without the device -- the cold start's grid, the screen walk, the gates, where the loop stands -- is solve_plan.hpp's.
#pragma once

// _cdPass! (coordinate_descent.jl:94-110)
// Screening of a FULL pass (exact, no reference counterpart).  A visit of a coordinate with
// beta_k == 0 leaves everything unchanged unless |X_k'r| exceeds its threshold (LS: lambda n w_k,
// cd_differentiable_function.jl:101-104 with x[k] == 0; SQRT: lambda w_k ||r||, :276), and as long
// as nothing moves r does not change -- so one pass over S columns that only takes their dots
// settles a whole run of such visits, and the Gram machinery is started at the first visit that
// can move.  Same iterates as visiting one by one; a full pass over a sparse iterate then reads X
// about once, at the plain streaming rate.  A 1e-9 relative margin sends borderline coordinates
// through the exact path.  After a hit the next `cool` visits are not screened (doubling on
// repeated hits), so a pass in which everything moves pays for a handful of screens only; a screen
// that settles all of its columns doubles the next one (64 -> 1024 columns: one host round trip per
// screen, so long quiet stretches run at the plain streaming rate of k_col_dots).  Which visits are
// screened and which streamed: ScreenWalk (solve_plan.hpp).
int32_t screened_full_pass(cdh_handle h, const int64_t* idx0, int64_t m, double* maxH) {
    {   // from the gradient cache when it is engaged: no read of X for the settled visits at all
        bool handled = false;
        CHK(gc_full_pass(h, idx0, m, maxH, &handled));
        if (handled) return CDH_OK;
    }
    GcThresholds T(h, 0.0);           // (no certificate: the dots are fresh)
    std::vector<double> cd;
    cd.reserve((size_t)(2 * ScreenWalk::longest_screen()));
    ScreenWalk walk(m, (h->mode == CDH_SWEEP_BLOCK) ? h->blockB : 1, h->cap, h->p);
    while (!walk.done()) {
        const ScreenStep s = walk.next();
        if (!s.screen) {
            CHK(run_chunk(h, idx0 + s.pos, s.len, maxH));
            continue;
        }
        const int S = s.len;
        const int64_t* visit = idx0 + s.pos;
        std::memcpy(h->h_idx, visit, sizeof(int64_t) * (size_t)S);
        HIPCHK(h, hipMemcpyAsync(h->d_idx, h->h_idx, sizeof(int64_t) * (size_t)S, hipMemcpyHostToDevice, h->stream));
        CHK(col_dots(h, 0, S, h->r, h->has_w, h->d_idx));   // X_k'W r, X_k'W X_k with observation weights
        CHK(queue_col_pairs(h, S, cd));
        if (h->loss == CDH_SQRT) {
            CHK(resid_moments_dev(h));
            CHK(queue_resid_sums(h));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->loss == CDH_SQRT) T.rnorm = std::sqrt(resid_sums(h).sumsq);
        const ColPairs xr(cd);
        int hit = S;
        for (int i = 0; i < S; ++i) {
            const int64_t k = visit[i];
            // a zero column (a == 0) goes to the exact path too: the reference turns it into NaN
            if (h->x.get(k) != 0.0 || !(std::fabs(xr.dot(i)) <= T.thr_of(k)) || !(xr.sq(i) > 0.0)) { hit = i; break; }
        }
        for (int i = 0; i < hit; ++i) replay_settled(h, visit[i], xr.dot(i) != 0.0);   // the first `hit` visits of the screen are settled
        walk.hit(hit);
    }
    return CDH_OK;
}

// _cdPass! (coordinate_descent.jl:94-110)
int32_t run_pass(cdh_handle h, const int64_t* idx0, int64_t m, double* maxH, bool screen = false) {
    *maxH = 0.0;
    if (screen && full_pass_screened(h, m)) {
        CHK(screened_full_pass(h, idx0, m, maxH));
    } else {
        for (int64_t off = 0; off < m; off += h->cap) {
            const int mm = (int)std::min<int64_t>(h->cap, m - off);
            // an active pass while the gradient cache holds the support's Gram columns: no read of X at all
            if (gc_ready_for_cov(h, idx0 + off, mm)) CHK(cov_chunk(h, idx0 + off, mm, maxH));
            else CHK(run_chunk(h, idx0 + off, mm, maxH));
        }
    }
    h->x.dropzeros();
    return CDH_OK;
}

// _coordinateDescent! (coordinate_descent.jl:65-92)
int32_t solve(cdh_handle h, const cdh_options* o, cdh::VisitScheduler& sched, cdh_stats* st) {
    SolveProgress at;
    std::vector<int64_t> visit;
    st->converged = 0;
    while (at.iter < o->maxIter) {
        // while the gradient cache can serve the passes, the loop itself runs on the device (cov_solve.hpp): one host round
        // trip per solve; what comes back is where the state machine stands
        {
            int outcome = kCsNotNow;
            CHK(cov_solve(h, o, sched, st, at, &outcome));
            if (outcome == kCsFinished) break;
            if (outcome == kCsAgain) continue;
        }
        const bool full = at.converged;
        sched.next_pass(h->x, full, visit);
        double maxH = 0.0;
        if (!visit.empty()) CHK(run_pass(h, visit.data(), (int64_t)visit.size(), &maxH, full));
        else h->x.dropzeros();
        h->gc.st.unprepared();
        st->passes += 1; st->visits += (int64_t)visit.size(); st->maxH = maxH;
        if (full) st->full_passes += 1;
        if (at.pass_done(maxH, o->optTol)) { st->converged = 1; break; }
    }
    st->domain_error = h->domain_error ? 1 : 0;
    return CDH_OK;
}

// _findLambdaMax (coordinate_descent.jl:118-149): col_stats.hpp, with the statistics it shares its read-backs with (declared
// ahead, as rebuild_residual_from is: the cold start below calls it)
int32_t lambda_max(cdh_handle h, double* out, std::vector<double>* dots = nullptr /* the (X_k'r, a_k) pairs, for a caller that can use them */);

// ---- the bodies of the exports ---------------------------------------------------------------------------------------------------
int32_t descend(cdh_handle h, int64_t k1, double* out_h) {
    CHK(check_coordinate(h, k1));
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t k0 = k1 - 1;
    double maxH = 0.0;
    const int save_mode = h->mode;
    h->mode = CDH_SWEEP_COORD;
    int32_t rc = run_chunk(h, &k0, 1, &maxH);  // no dropzeros!: that is _cdPass!'s job
    h->mode = save_mode;
    if (rc != CDH_OK) return rc;
    if (out_h) *out_h = h->h_hs[0];
    return CDH_OK;
}

int32_t pass(cdh_handle h, int64_t m, const int64_t* idx1, double* out_maxH) {
    if (m < 0) return fail(h, CDH_BAD_ARG, "m < 0");
    CHK(exchange_alive(h));
    if (m > 0) NEED_P(h, idx1);
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<int64_t> idx0((size_t)m);
    CHK(check_columns(h, idx1, m));
    for (int64_t i = 0; i < m; ++i) idx0[(size_t)i] = idx1[i] - 1;
    double maxH = 0.0;
    h->gc.st.unprepared();
    if (m > 0) CHK(run_pass(h, idx0.data(), m, &maxH, h->screening >= 2));
    else h->x.dropzeros();
    if (out_maxH) *out_maxH = maxH;
    return CDH_OK;
}

int32_t solve_once(cdh_handle h, const cdh_options* opt, cdh_stats* out) {
    NEED_P(h, opt);
    CHK(exchange_alive(h));
    HIPCHK(h, hipSetDevice(h->device));
    cdh_stats st{};
    if (small_applicable(h, opt)) {
        CHK(small_prepare(h));
        if (h->small.enabled) {     // (the preparation may find no room and switch the path off)
            uint64_t rng = opt->seed;
            const double lam = h->ctrl.lambda0;
            int32_t rcs = small_solve(h, opt, &lam, 1, &rng, &st, false);
            if (rcs != kSmallPrecisionLost) {
                if (out) *out = st;
                return rcs;
            }
            st = cdh_stats{};            // (r'r out of digits: the streamed kernels below take the call)
        }
    }
    cdh::VisitScheduler sched(h->p, opt->randomize != 0, opt->seed);
    const SmallRent rent(h, opt);
    int32_t rc = solve(h, opt, sched, &st);
    rent.pay(st);
    if (out) *out = st;
    return rc;
}

// The head of a cold start (coordinate_descent.jl:25-29), one-launch or streamed: fill!(x, 0), initialize!, _findLambdaMax at
// r = y, and the numSteps + 1 lambdas from there down to the caller's lambda0.
int32_t cold_start_grid_of(cdh_handle h, const cdh_options* opt, bool one_launch, cdh_stats* st, std::vector<double>& grid) {
    h->x.clear();                                       // fill!(x, 0)           (:25)
    double lmax = 0.0;
    if (one_launch) {
        HIPCHK(h, hipMemsetAsync(h->beta, 0, sizeof(double) * h->p, h->stream));
        // max_k |X_k'y| / n / omega_k (sqrt-lasso: / ||y||) -- from the cached X'y
        const double denom = h->loss == CDH_SQRT ? std::sqrt(h->small.yy) : (double)h->n_total;
        lmax = lambda_max_of(h->small.h_c.data(), 2, h->p, denom, h->has_omega ? h->h_omega.data() : nullptr);
    } else {
        CHK(rebuild_residual(h));                       // initialize!(f, x)     (:26)
        // 51 solves on the same X follow: the gradient cache (mode 1) need not wait for evidence
        h->gc.full_seen = std::max<int64_t>(h->gc.full_seen, 1000);
        std::vector<double> dots;
        CHK(lambda_max(h, &lmax, &dots));               // _findLambdaMax        (:29)
        CHK(gc_adopt_dots(h, dots));                    // ... whose pass over X is the cache's reference pass as well
    }
    st->lambda_max = lmax;
    grid.resize((size_t)opt->numSteps + 1);
    if (!cold_start_grid(lmax, h->ctrl.lambda0, opt->numSteps, grid.data()))
        return fail(h, CDH_BAD_ARG, "cold start: the range log(lambda_max):step:log(lambda0) has a zero step");
    return CDH_OK;
}

// coordinateDescent! (coordinate_descent.jl:7-39)
int32_t coordinate_descent(cdh_handle h, const cdh_options* opt, cdh_stats* out) {
    NEED_P(h, opt);
    CHK(exchange_alive(h));
    HIPCHK(h, hipSetDevice(h->device));
    cdh_stats st{};
    cdh::VisitScheduler sched(h->p, opt->randomize != 0, opt->seed);
    h->domain_error = false;
    int32_t rc = CDH_OK;
    bool small = small_applicable(h, opt, !opt->warmStart);   // a cold start is numSteps + 1 solves: it buys the Gram form outright
    if (small) { CHK(small_prepare(h)); small = h->small.enabled; }
    const SmallRent rent(h, opt);
    uint64_t rng = opt->seed;       // the one-launch solve carries the scheduler's generator state itself
    std::vector<double> grid;
    // ---- in one launch (small_solve.hpp) where the Gram form applies -- unless its r'r runs out of digits (kSmallPrecisionLost:
    // nothing of the launch is used), in which case the streamed kernels below take the call ----
    if (small && opt->warmStart) {
        // initialize!(f, x) (:21) makes r = y - X x by definition: the one-launch solve derives its gradient from that
        // identity (g = X'y - G x) and leaves the residual to be formed when somebody reads it
        const double lam = h->ctrl.lambda0;
        rc = small_solve(h, opt, &lam, 1, &rng, &st, true);
    } else if (small) {
        CHK(cold_start_grid_of(h, opt, true, &st, grid));
        rc = small_solve(h, opt, grid.data(), (int)grid.size(), &rng, &st, true);   // the numSteps + 1 solves of (:32-36) inside one launch
    }
    if (small && rc == kSmallPrecisionLost) { small = false; st = cdh_stats{}; rc = CDH_OK; }
    if (small) {
        // done above
    } else if (opt->warmStart) {
        // initialize!(f, x) (:21).  Optional shortcut for warm-started paths (LassoPath): the
        // carried residual already equals y - X beta, so the rebuild only re-rounds it.
        if (!(h->reuse_residual && h->rs.consistent())) CHK(rebuild_residual(h));
        rc = solve(h, opt, sched, &st);
    } else {
        const double target = h->ctrl.lambda0;          // g itself is never mutated by the reference:
        rc = [&]() -> int32_t {                         // whatever happens below, lambda0 is put back
            CHK(cold_start_grid_of(h, opt, false, &st, grid));
            for (const double lambda : grid) {          // (:32-36)
                h->ctrl.lambda0 = lambda;
                CHK(solve(h, opt, sched, &st));
            }
            return CDH_OK;
        }();
        h->ctrl.lambda0 = target;
        if (rc == CDH_OK) {
            CHK(upload_ctrl(h));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
    }
    if (!small) rent.pay(st);
    if (out) *out = st;
    return rc;
}
