// quad_solve.hpp -- CDQuadraticLoss (cd_differentiable_function.jl:299-348: f(x) = x'Ax/2 + x'b) for a BATCH of problems that
// share A: a section of cdhip.hip kept in its own file (included once, inside cdhip.hip's anonymous namespace, after
// small_solve.hpp, whose scheduler, dropzeros! and generator it calls).
//
// Why: one covariance-form problem with p <= ~2000 occupies one wave (small_solve.hpp: on par with one CPU core).  But such
// problems come many at a time on one A -- the p neighbourhood regressions of a graph (b = -A_j, coordinate j penalised
// infinitely), CLIME columns, grids of lambda, many right-hand sides -- and one workgroup per problem on 256 CUs, with A
// resident in L2 / Infinity Cache, is work for the whole chip.
//
// How: k_quad_solve runs coordinateDescent! / _coordinateDescent! / _cdPass! (coordinate_descent.jl:7-39, 65-110) for problem
// blockIdx.x: its g = A x + b, beta, 1 / diag(A), omega, visit list, support slots and the shuffle's scratch stay in dynamic
// LDS for the whole solve (quad_solve_types.hpp: the layout, CDH_QUAD_MAX_P); a move reads its column of A from device memory.
// A workgroup leaves on its own `prev_converged && converged` or maxIter and shares nothing with the others.
//
// The workgroup is ONE wave (kQuadThreads = 64), and that follows from the code it runs: wave_build_list and wave_dropzeros
// (small_solve.hpp) are written for one wave -- their only synchronisation is the wave's own in-order LDS -- and the visits are
// a serial chain in which each step waits for the ballot of the one before it, so further waves would idle through everything
// but the g += h A_k update of a move.  The chip is filled by problems, not by threads: the LDS a problem takes (64 p bytes)
// decides how many share a CU -- twelve at p = 200, two at p = 1000 -- and while one wave waits for its column of A the
// others visit.
#pragma once

struct QuadArgs {
    int32_t p, nlam, randomize, has_omega;
    int64_t ldo;                         // omega of problem j: omega + j ldo (0: one vector for all)
    int64_t lam_stride;                  // lambdas of problem j: lambdas + j lam_stride, nlam of them
    int64_t maxIter;
    double optTol;
    uint64_t seed;
    const double *A, *inv_a, *omega, *lambdas;
    double *beta, *g;                    // p per problem
    int32_t *sup, *nnz;                  // the support in slot order (p per problem), its length
    QuadStat* stats;
    // the explicit-list instantiation: one pass of problem `problem` over list[0 .. nlist) (0-based), then dropzeros! if asked
    const int32_t* list;
    int32_t nlist, dropzeros, problem;
    double* h_out;                       // the signed h of the list's last visit (descendCoordinate!)
};

// _cdPass! (coordinate_descent.jl:94-110) over list[0 .. L), the visit being CDQuadraticLoss's (:324-348):
//   a = 1 / A_kk,  x_k <- S(x_k - g_k a, a lambda0 omega_k),  on a move g += h A[:, k].
// 64 consecutive positions are evaluated at once against the current g; the positions before the first one that moves are
// settled exactly (g changes only when something moves), that one is applied, and the rest are evaluated again.
// DUPS: the list is a caller's and may name a coordinate twice -- a chunk then ends before the repeat, so that no two lanes of
// a step hold the same coordinate (the scheduler's lists are permutations).  Returns max |h|; *h_last = the last visit's h.
template <bool DUPS>
__device__ __forceinline__ double quad_pass(int lane, int p, const int32_t* list, int L, double lambda0, const double* __restrict__ A,
                                            double* s_g, double* s_beta, const double* s_ia, const double* s_om,
                                            int32_t* s_slot2ind, int32_t* s_ind2slot, int& nnz, double* h_last) {
    const unsigned long long below = (1ull << lane) - 1ull;
    double maxH = 0.0, hl = 0.0;
    for (int c0 = 0; c0 < L;) {
        int clen = min(64, L - c0);
        const int k = lane < clen ? list[c0 + lane] : 0;
        if constexpr (DUPS) {
            bool dup = false;
            for (int t = 0; t + 1 < clen; ++t) { const int kt = __shfl(k, t, 64); dup |= t < lane && lane < clen && kt == k; }
            const unsigned long long dm = __ballot(dup);
            if (dm) clen = min(clen, (int)__builtin_ctzll(dm));          // (lane 0 repeats nothing: clen stays >= 1)
        }
        const bool valid = lane < clen;
        const double ia = s_ia[k];
        const double thr = ia * lambda0 * s_om[k];                       // cdprox!(g, x, k, a): gamma lambda0 omega_k
        int done = 0;
        for (;;) {
            const double oldv = s_beta[k], gk = s_g[k];
            const int islot = s_ind2slot[k];
            const double v = oldv - gk * ia;
            const double nv = soft_threshold(v, thr);
            const double hh = nv - oldv;
            const bool moves = valid && lane >= done && !(hh == 0.0);    // a NaN step "moves" (it propagates, as in the reference)
            const unsigned long long mmask = __ballot(moves);
            const int first = __builtin_amdgcn_readfirstlane(mmask ? (int)__builtin_ctzll(mmask) : 64);
            // SparseIterate bookkeeping of the settled visits [done, first), in order: a pre-prox non-zero appends a slot
            // (x[k] = x[k] - b a), cdprox! then stores the unchanged value
            {
                const bool app = valid && lane >= done && lane < first && v != 0.0 && islot == 0;
                const unsigned long long amask = __ballot(app);
                if (app) { const int sl = nnz + __popcll(amask & below); s_slot2ind[sl] = k; s_ind2slot[k] = sl + 1; }
                nnz += __popcll(amask);
            }
            if (first >= 64) { if (done < clen) hl = 0.0; break; }      // the rest of the chunk stays where it is
            // ---- the visit that moves: broadcast from its lane ----
            const int km = __builtin_amdgcn_readlane(k, first);
            const double nvm = readlane_f64(nv, first), h = readlane_f64(hh, first);
            const int pre_nz = __builtin_amdgcn_readlane((int)(v != 0.0), first);
            const bool appm = __builtin_amdgcn_readlane(islot, first) == 0 && (pre_nz != 0 || nvm != 0.0);
            if (lane == first) {
                if (appm) { s_slot2ind[nnz] = km; s_ind2slot[km] = nnz + 1; }
                s_beta[km] = nvm;
            }
            if (appm) nnz += 1;
            const double ah = fabs(h);
            if (ah > maxH) maxH = ah;                                    // a NaN h never raises maxH (coordinate_descent.jl:104)
            hl = first == clen - 1 ? h : 0.0;
            const double* __restrict__ col = A + (int64_t)km * p;        // A is symmetric (the caller's contract, :306): row k = column k
#pragma unroll 4
            for (int j = lane; j < p; j += 64) s_g[j] = fma(h, col[j], s_g[j]);
            CDH_WAVE_SYNC();
            done = first + 1;
            if (done >= clen) break;
        }
        CDH_WAVE_SYNC();
        c0 += clen;
    }
    *h_last = hl;
    return maxH;
}

template <bool EXPLICIT>
__global__ __launch_bounds__(kQuadThreads) void k_quad_solve(QuadArgs a) {
    extern __shared__ double s_dyn[];
    char* base = reinterpret_cast<char*>(s_dyn);
    const int p = a.p;
    const QuadLds lay = quad_lds_layout(p);
    double* s_g = reinterpret_cast<double*>(base + lay.g);
    double* s_beta = reinterpret_cast<double*>(base + lay.beta);
    double* s_ia = reinterpret_cast<double*>(base + lay.inv_a);
    double* s_om = reinterpret_cast<double*>(base + lay.omega);
    int32_t* s_list = reinterpret_cast<int32_t*>(base + lay.list);
    int32_t* s_slot2ind = reinterpret_cast<int32_t*>(base + lay.slot2ind);
    int32_t* s_ind2slot = reinterpret_cast<int32_t*>(base + lay.ind2slot);
    int32_t* s_order = reinterpret_cast<int32_t*>(base + lay.order);     // the shuffle; between passes: scratch of dropzeros!
    int32_t* s_draw = reinterpret_cast<int32_t*>(base + lay.draw);
    int32_t* s_fyoff = reinterpret_cast<int32_t*>(base + lay.fyoff);
    int32_t* s_fybucket = reinterpret_cast<int32_t*>(base + lay.fybucket);
    int32_t* s_fypar = reinterpret_cast<int32_t*>(base + lay.fypar);
    const int lane = threadIdx.x;
    const int64_t prob = EXPLICIT ? (int64_t)a.problem : (int64_t)blockIdx.x;
    double* __restrict__ beta = a.beta + prob * p;
    double* __restrict__ g = a.g + prob * p;
    int32_t* __restrict__ sup = a.sup + prob * p;
    const double* __restrict__ om = a.has_omega ? a.omega + prob * a.ldo : nullptr;
    const double* __restrict__ lam = a.lambdas + prob * a.lam_stride;
    int nnz = a.nnz[prob];
    for (int k = lane; k < p; k += 64) {
        s_g[k] = g[k]; s_beta[k] = beta[k]; s_ia[k] = a.inv_a[k];
        s_om[k] = om ? om[k] : 1.0;
        s_ind2slot[k] = 0;
    }
    __syncthreads();
    for (int s = lane; s < nnz; s += 64) { const int k = sup[s]; s_slot2ind[s] = k; s_ind2slot[k] = s + 1; }
    __syncthreads();
    int64_t passes = 0, full_passes = 0, visits = 0;
    int converged = 0;
    double lastH = 0.0, h_last = 0.0;
    if constexpr (EXPLICIT) {
        lastH = quad_pass<true>(lane, p, a.list, a.nlist, lam[0], a.A, s_g, s_beta, s_ia, s_om, s_slot2ind, s_ind2slot, nnz, &h_last);
        __syncthreads();
        if (a.dropzeros) nnz = wave_dropzeros(lane, nnz, s_beta, s_slot2ind, s_ind2slot, s_order, s_draw);
        passes = 1; visits = a.nlist;
    } else {
        uint64_t rng = a.seed;
        for (int il = 0; il < a.nlam; ++il) {
            const double lambda0 = lam[il];
            bool prev_conv = false, conv = true;
            converged = 0;
            for (int64_t iter = 0; iter < a.maxIter; ++iter) {
                const bool full = conv;
                const int L = wave_build_list(lane, full, a.randomize, p, nnz, rng, s_order, s_draw, s_list, s_slot2ind, s_fyoff,
                                              s_fybucket, s_fypar);
                const double maxH = quad_pass<false>(lane, p, s_list, L, lambda0, a.A, s_g, s_beta, s_ia, s_om, s_slot2ind,
                                                     s_ind2slot, nnz, &h_last);
                __syncthreads();
                nnz = wave_dropzeros(lane, nnz, s_beta, s_slot2ind, s_ind2slot, s_order, s_draw);
                __syncthreads();
                passes += 1; visits += L; lastH = maxH;
                if (full) full_passes += 1;
                prev_conv = conv;
                conv = maxH < a.optTol;
                if (prev_conv && conv) { converged = 1; break; }
            }
        }
    }
    __syncthreads();
    for (int k = lane; k < p; k += 64) { beta[k] = s_beta[k]; g[k] = s_g[k]; }
    for (int s = lane; s < nnz; s += 64) sup[s] = s_slot2ind[s];
    if (lane == 0) {
        a.nnz[prob] = nnz;
        QuadStat st;
        st.passes = passes; st.full_passes = full_passes; st.visits = visits; st.converged = converged; st.nnz = nnz; st.maxH = lastH;
        a.stats[prob] = st;
        if constexpr (EXPLICIT) *a.h_out = h_last;
    }
}

// initialize!(f, x) (cd_differentiable_function.jl:311-320) for every problem: g_j = b_j + sum_s beta_s A[:, s], the sum in slot
// order as the reference's A_mul_B_row takes it.  One workgroup per problem, a thread per row.
__global__ __launch_bounds__(256) void k_quad_init(int p, const double* __restrict__ A, const double* __restrict__ B,
                                                   const double* __restrict__ beta, const int32_t* __restrict__ sup,
                                                   const int32_t* __restrict__ nnz, double* __restrict__ g) {
    const int64_t off = (int64_t)blockIdx.x * p;
    const int n = nnz[blockIdx.x];
    for (int i = threadIdx.x; i < p; i += 256) {
        double acc = 0.0;
        for (int s = 0; s < n; ++s) { const int ks = sup[off + s]; acc += A[(int64_t)ks * p + i] * beta[off + ks]; }
        g[off + i] = acc + B[off + i];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// (a quad handle has no error string of its own: what goes wrong on it is reported where cdh_last_error(NULL) finds it)
inline int32_t quad_fail(int32_t code, const char* msg) { g_create_error = msg; return code; }
#define QCHK(call)                                                                                              \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            char buf_[512];                                                                                     \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            g_create_error = buf_;                                                                              \
            return e_ == hipErrorOutOfMemory ? CDH_OOM : CDH_HIP_ERROR;                                         \
        }                                                                                                       \
    } while (0)
#define QNEED(cond, msg)                                             \
    do {                                                             \
        if (!(cond)) return quad_fail(CDH_BAD_ARG, msg);             \
    } while (0)
#define QREFUSE(expr)                                                \
    do {                                                             \
        const char* m_ = (expr);                                     \
        if (m_) return quad_fail(CDH_BAD_ARG, m_);                   \
    } while (0)

void quad_free(cdh_quad q) {
    if (!q) return;
    (void)hipSetDevice(q->device);
    const hipStream_t stream = q->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete q;                              // the owners free the device and pinned memory before the stream goes
    if (stream) (void)hipStreamDestroy(stream);
}

struct QuadOwner {                         // cdh_quad_create's hold on the handle while it is being built
    cdh_quad q;
    ~QuadOwner() { quad_free(q); }
    cdh_quad release() { cdh_quad r = q; q = nullptr; return r; }
};

// every buffer of the handle, all or nothing: on a failure the half-built set is dropped and the handle holds none
int32_t quad_alloc(cdh_quad q) {
    const size_t p = (size_t)q->p, mb = (size_t)q->max_batch;
    DevBuf<double> A, inv_a, B, omega, lambda0, grid, beta, g, h_out;
    DevBuf<int32_t> sup, nnz;
    DevBuf<QuadStat> stats;
    PinBuf<QuadStat> h_stats;
    PinBuf<double> h_h;
    QCHK(A.alloc(sizeof(double) * p * p));
    QCHK(inv_a.alloc(sizeof(double) * p));
    QCHK(B.alloc(sizeof(double) * p * mb));
    QCHK(omega.alloc(sizeof(double) * p * mb));
    QCHK(lambda0.alloc(sizeof(double) * mb));
    QCHK(grid.alloc(sizeof(double) * mb * kQuadMaxLam));
    QCHK(beta.alloc(sizeof(double) * p * mb));
    QCHK(g.alloc(sizeof(double) * p * mb));
    QCHK(h_out.alloc(sizeof(double)));
    QCHK(sup.alloc(sizeof(int32_t) * p * mb));
    QCHK(nnz.alloc(sizeof(int32_t) * mb));
    QCHK(stats.alloc(sizeof(QuadStat) * mb));
    QCHK(h_stats.alloc(sizeof(QuadStat) * mb));
    QCHK(h_h.alloc(sizeof(double)));
    q->A = std::move(A); q->inv_a = std::move(inv_a); q->B = std::move(B); q->omega = std::move(omega);
    q->lambda0 = std::move(lambda0); q->grid = std::move(grid); q->beta = std::move(beta); q->g = std::move(g);
    q->h_out = std::move(h_out); q->sup = std::move(sup); q->nnz = std::move(nnz); q->stats = std::move(stats);
    q->h_stats = std::move(h_stats); q->h_h = std::move(h_h);
    return CDH_OK;
}

QuadArgs quad_args(cdh_quad q) {
    QuadArgs a{};
    a.p = (int32_t)q->p; a.nlam = 1; a.has_omega = q->has_omega ? 1 : 0; a.ldo = q->omega_shared ? 0 : q->p;
    a.lam_stride = 1; a.lambdas = q->lambda0;
    a.A = q->A; a.inv_a = q->inv_a; a.omega = q->omega; a.beta = q->beta; a.g = q->g; a.sup = q->sup; a.nnz = q->nnz;
    a.stats = q->stats; a.h_out = q->h_out;
    return a;
}

// what the exports that run something need: A, b and the penalty in place
int32_t quad_ready(cdh_quad q, bool penalty) {
    QNEED(q->A_set, "cdh_quad_set_A has not been called");
    QNEED(q->m > 0, "no problems are loaded: cdh_quad_set_b first");
    if (penalty) QNEED(q->penalty_set, "cdh_quad_set_penalty has not been called since cdh_quad_set_b");
    QCHK(hipSetDevice(q->device));
    return CDH_OK;
}

// the iterates as the device holds them, fetched once after whatever changed them
int32_t quad_pull(cdh_quad q) {
    if (!q->host_stale) return CDH_OK;
    const size_t p = (size_t)q->p, m = (size_t)q->m;
    q->h_beta.resize(p * m); q->h_sup.resize(p * m); q->h_nnz.resize(m);
    QCHK(hipMemcpyAsync(q->h_beta.data(), q->beta, sizeof(double) * p * m, hipMemcpyDeviceToHost, q->stream));
    QCHK(hipMemcpyAsync(q->h_sup.data(), q->sup, sizeof(int32_t) * p * m, hipMemcpyDeviceToHost, q->stream));
    QCHK(hipMemcpyAsync(q->h_nnz.data(), q->nnz, sizeof(int32_t) * m, hipMemcpyDeviceToHost, q->stream));
    QCHK(hipStreamSynchronize(q->stream));
    q->host_stale = false;
    return CDH_OK;
}

// one pass of problem j over an explicit 1-based list; dropzeros! after it unless this is a lone descendCoordinate!
int32_t quad_explicit(cdh_quad q, int64_t j, int64_t n, const int64_t* idx1, bool dropzeros, double* maxH, double* h_last) {
    CHK(quad_ready(q, true));
    QREFUSE(quad_check_problem(j, q->m));
    QNEED(n >= 0 && n <= ((int64_t)1 << 30), "the visit list's length must be in 0 .. 2^30");
    QNEED(n == 0 || idx1, "idx1 is NULL");
    std::vector<int32_t> list((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        QNEED(idx1[i] >= 1 && idx1[i] <= q->p, "a coordinate of the visit list is outside 1 .. p");
        list[(size_t)i] = (int32_t)(idx1[i] - 1);
    }
    if (n > q->list_cap) {
        DevBuf<int32_t> bigger;
        QCHK(bigger.alloc(sizeof(int32_t) * (size_t)n));
        q->list = std::move(bigger);
        q->list_cap = n;
    }
    if (n) QCHK(hipMemcpyAsync(q->list, list.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, q->stream));
    QuadArgs a = quad_args(q);
    a.list = q->list; a.nlist = (int32_t)n; a.dropzeros = dropzeros ? 1 : 0; a.problem = (int32_t)j;
    hipLaunchKernelGGL(k_quad_solve<true>, dim3(1), dim3(kQuadThreads), q->lds_bytes, q->stream, a);
    QCHK(hipGetLastError());
    QCHK(hipMemcpyAsync(q->h_stats, q->stats + j, sizeof(QuadStat), hipMemcpyDeviceToHost, q->stream));
    QCHK(hipMemcpyAsync(q->h_h, q->h_out, sizeof(double), hipMemcpyDeviceToHost, q->stream));
    QCHK(hipStreamSynchronize(q->stream));
    q->host_stale = true;
    if (maxH) *maxH = q->h_stats[0].maxH;
    if (h_last) *h_last = q->h_h[0];
    return CDH_OK;
}

// coordinateDescent! (coordinate_descent.jl:7-39) for all m problems: initialize! (or the cold start's zero iterate and
// lambda grids) and ONE launch of k_quad_solve; the statistics come back in one copy
int32_t quad_coordinate_descent(cdh_quad q, const cdh_options* o, cdh_stats* out) {
    CHK(quad_ready(q, true));
    QREFUSE(quad_check_options(o->maxIter, o->warmStart, o->numSteps));
    const size_t p = (size_t)q->p, m = (size_t)q->m;
    QuadArgs a = quad_args(q);
    a.randomize = o->randomize ? 1 : 0; a.maxIter = o->maxIter; a.optTol = o->optTol; a.seed = o->seed;
    std::vector<double> lmax(m, 0.0);
    if (o->warmStart) {
        hipLaunchKernelGGL(k_quad_init, dim3((unsigned)m), dim3(256), 0, q->stream, (int)q->p, q->A, q->B, q->beta, q->sup, q->nnz, q->g);
        QCHK(hipGetLastError());
    } else {
        // fill!(x, 0); initialize!: g = b (:25-26); _findLambdaMax (:29) = max_k |b_k| / omega_k; the numSteps + 1 solves down the
        // log grid (:32-36) inside the launch
        std::vector<double> grid(m * kQuadMaxLam, 0.0);
        for (size_t j = 0; j < m; ++j) {
            const double* om = q->has_omega ? q->h_omega.data() + (q->omega_shared ? 0 : j * p) : nullptr;
            lmax[j] = lambda_max_of(q->h_B.data() + j * p, 1, q->p, 1.0, om);
            if (!cold_start_grid(lmax[j], q->h_lambda0[j], o->numSteps, grid.data() + j * kQuadMaxLam))
                return quad_fail(CDH_BAD_ARG, "cold start: the range log(lambda_max):step:log(lambda0) of a problem has a zero step");
        }
        QCHK(hipMemcpyAsync(q->grid, grid.data(), sizeof(double) * grid.size(), hipMemcpyHostToDevice, q->stream));
        QCHK(hipStreamSynchronize(q->stream));        // (grid is a local: the copy has read it before it goes)
        QCHK(hipMemsetAsync(q->beta, 0, sizeof(double) * p * m, q->stream));
        QCHK(hipMemsetAsync(q->nnz, 0, sizeof(int32_t) * m, q->stream));
        QCHK(hipMemcpyAsync(q->g, q->B, sizeof(double) * p * m, hipMemcpyDeviceToDevice, q->stream));
        a.lambdas = q->grid; a.lam_stride = kQuadMaxLam; a.nlam = (int32_t)(o->numSteps + 1);
    }
    q->host_stale = true;
    hipLaunchKernelGGL(k_quad_solve<false>, dim3((unsigned)m), dim3(kQuadThreads), q->lds_bytes, q->stream, a);
    QCHK(hipGetLastError());
    QCHK(hipMemcpyAsync(q->h_stats, q->stats, sizeof(QuadStat) * m, hipMemcpyDeviceToHost, q->stream));
    QCHK(hipStreamSynchronize(q->stream));
    for (size_t j = 0; j < m && out; ++j) {
        const QuadStat& s = q->h_stats[j];
        cdh_stats st{};
        st.passes = s.passes; st.full_passes = s.full_passes; st.visits = s.visits; st.converged = s.converged; st.maxH = s.maxH;
        st.lambda_max = lmax[j];
        out[j] = st;
    }
    return CDH_OK;
}
