// cv_path.hpp -- K-fold cross-validation of a lasso path (no reference counterpart; the solves are LassoPath's, lasso.jl:229-260,
// on the weighted loss with 0/1 weights and the scales of _stdX!(w, X), utils.jl:140-151): the fold ids of the rows resident on
// the device, a fold's 0/1 observation weights written from them, and the sums of squared prediction errors of a whole path's
// coefficients over the held-out and the training rows in one pass over the columns involved.  Included by cdhip.hip inside its
// anonymous namespace, after the handle; sizes, limits and layouts are cv_plan.hpp's.

// w_i = (fold_i == k ? 0 : 1) in the handle's dtype; fold == nullptr (k == -1): all ones.  Rows [n, ld) stay zero.
template <typename T>
__global__ __launch_bounds__(256) void k_fold_weights(T* __restrict__ w, const uint8_t* __restrict__ fold, int64_t n, int k) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        w[i] = (fold && (int)fold[i] == k) ? (T)0 : (T)1;
}

// One group of kCvGroup coefficient columns over all rows.  A lane owns a row: acc[j] = y_i - sum_t X[i, idx[t]] Bg[t, j], every
// term an fp64 FMA, the columns of X walked once, kCvUnroll loads in flight; Bg (the group's [srows][kCvGroup] slice of the
// packed image, rows s .. srows - 1 zero) and idx are wave-uniform, so they come through the scalar cache and the FMAs take them
// as scalar operands.  The squares then leave the lanes through LDS, kCvChunk columns at a time, and lane (c, q) adds rows
// q, q + 16, ... of column c to its held or its training sum by the row's fold; after the last tile the 16 lanes of a column
// are summed by a fixed butterfly and the workgroup's record goes to partials[blockIdx.x * nvals + ...]: [held][train] at
// col0 + column.  Every order is fixed: bit-identical run to run.  Rows beyond n are loaded clamped and contribute zeros.
// 2 waves per SIMD: the 128 accumulator registers leave room for no more than three, and the compiler is told not to trade
// occupancy for spills.
template <typename T>
__global__ __launch_bounds__(kCvRows, 2) void k_path_sse(const T* __restrict__ X, int64_t ld, int64_t n, const T* __restrict__ y,
                                                        const uint8_t* __restrict__ fold, int k,
                                                        const int64_t* __restrict__ idx, int s, int srows,
                                                        const double* __restrict__ Bg, double* __restrict__ partials,
                                                        int nvals, int mpad, int col0) {
    __shared__ double s_t[kCvChunk * kCvStride];
    constexpr int NCH = kCvGroup / kCvChunk;
    const int tid = threadIdx.x, c = tid >> 4, q = tid & 15;
    double hs[NCH], ts[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) { hs[ch] = 0.0; ts[ch] = 0.0; }
    const int64_t ntiles = (n + kCvRows - 1) / kCvRows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {      // (the same trips for every lane of the workgroup)
        const int64_t row0 = tile * kCvRows, i = row0 + tid;
        const bool live = i < n;
        const int64_t ii = live ? i : n - 1;
        double acc[kCvGroup];
        const double yi = (double)y[ii];
#pragma unroll
        for (int j = 0; j < kCvGroup; ++j) acc[j] = yi;
        for (int t0 = 0; t0 < srows; t0 += kCvUnroll) {
            double x[kCvUnroll];
#pragma unroll
            for (int u = 0; u < kCvUnroll; ++u) {
                const int t = t0 + u < s ? t0 + u : s - 1;                   // (the address is clamped, the load unconditional)
                x[u] = (double)X[idx[t] * ld + ii];
            }
#pragma unroll
            for (int u = 0; u < kCvUnroll; ++u) {
                const double xv = t0 + u < s ? -x[u] : 0.0;
                const double* __restrict__ b = Bg + (int64_t)(t0 + u) * kCvGroup;
#pragma unroll
                for (int j = 0; j < kCvGroup; ++j) acc[j] = fma(xv, b[j], acc[j]);
            }
        }
        // which of this lane's 16 rows of the tile are held out
        unsigned held = 0;
        if (fold && k >= 0) {
            int id[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {                                     // (clamped addresses, unconditional loads)
                const int64_t r = row0 + q + 16 * u;
                id[u] = (int)fold[r < n ? r : n - 1];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) held |= (row0 + q + 16 * u < n && id[u] == k) ? 1u << u : 0u;
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            __syncthreads();                                                   // the previous chunk has been read
#pragma unroll
            for (int jj = 0; jj < kCvChunk; ++jj) {
                const double v = acc[ch * kCvChunk + jj];
                s_t[jj * kCvStride + tid] = live ? v * v : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const double v = s_t[c * kCvStride + q + 16 * u];
                if ((held >> u) & 1u) hs[ch] += v; else ts[ch] += v;
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            hs[ch] += __shfl_xor(hs[ch], off, 16);
            ts[ch] += __shfl_xor(ts[ch], off, 16);
        }
        if (q == 0) {
            double* rec = partials + (int64_t)blockIdx.x * nvals + col0 + ch * kCvChunk + c;
            rec[0] = hs[ch];
            rec[mpad] = ts[ch];
        }
    }
}

int32_t cv_refuse_shards(cdh_handle h) {
    if (h->n != h->n_total || h->xs.sharded())
        return fail(h, CDH_BAD_ARG, "folds and cdh_path_sse do not run on row-sharded handles");
    return CDH_OK;
}

// the scratch of cdh_path_sse, allocated by the first call, all or nothing; B's image grows with the largest call
int32_t cv_scratch(cdh_handle h, int64_t b_doubles) {
    CvState& cv = h->cv;
    if (!cv.ready) {
        DevBuf<double> partials, out;
        DevBuf<int64_t> idx;
        HIPCHK(h, partials.alloc(sizeof(double) * (size_t)kCvPartialDoubles));
        HIPCHK(h, out.alloc(sizeof(double) * (size_t)kCvMaxVals));
        HIPCHK(h, idx.alloc(sizeof(int64_t) * (size_t)kCvMaxS));
        cv.partials = std::move(partials); cv.out = std::move(out); cv.idx = std::move(idx);
        cv.ready = true;
    }
    if (b_doubles > cv.b_cap) {
        DevBuf<double> B;
        HIPCHK(h, B.alloc(sizeof(double) * (size_t)b_doubles));
        cv.B = std::move(B);          // (the swap hands the old image to B, which frees it)
        cv.b_cap = b_doubles;
    }
    return CDH_OK;
}

int32_t cv_set_folds(cdh_handle h, const int32_t* fold_of_row, int32_t K, int64_t* out_count) {
    CHK(cv_refuse_shards(h));
    CvState& cv = h->cv;
    if (!fold_of_row && K == 0) {
        DevBuf<uint8_t> none;
        cv.fold = std::move(none);
        cv.K = 0;
        return CDH_OK;
    }
    NEED_P(h, fold_of_row);
    if (const char* why = cv_check_K(h->n, K)) return fail(h, CDH_BAD_ARG, why);
    std::vector<uint8_t> ids((size_t)h->n);
    std::vector<int64_t> count((size_t)K, 0);
    for (int64_t i = 0; i < h->n; ++i) {
        const int32_t f = fold_of_row[i];
        if (f < 0 || f >= K) {
            char buf[128];
            snprintf(buf, sizeof buf, "fold_of_row[%lld] = %d is outside 0 .. K - 1", (long long)i, (int)f);
            return fail(h, CDH_BAD_ARG, buf);
        }
        ids[(size_t)i] = (uint8_t)f;
        ++count[(size_t)f];
    }
    for (int32_t f = 0; f < K; ++f)
        if (count[(size_t)f] == 0) {
            char buf[64];
            snprintf(buf, sizeof buf, "fold %d is empty", (int)f);
            return fail(h, CDH_BAD_ARG, buf);
        }
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<uint8_t> fold;
    HIPCHK(h, fold.alloc((size_t)h->n));
    HIPCHK(h, hipMemcpyAsync(fold, ids.data(), (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    cv.fold = std::move(fold);
    cv.K = K;
    if (out_count) for (int32_t f = 0; f < K; ++f) out_count[f] = count[(size_t)f];
    return CDH_OK;
}

// what cdh_set_fold_weights refuses, before the handle is touched
int32_t cv_check_fold_weights(cdh_handle h, int32_t k) {
    CHK(cv_refuse_shards(h));
    if (h->loss != CDH_WLS) return fail(h, CDH_BAD_ARG, "observation weights need the CDH_WLS loss");
    if (k < -1) return fail(h, CDH_BAD_ARG, "k must be a fold, or -1 for all ones");
    if (k >= 0 && h->cv.K == 0) return fail(h, CDH_BAD_ARG, "k >= 0 needs cdh_set_folds first");
    if (k >= h->cv.K && k >= 0) return fail(h, CDH_BAD_ARG, "k must be below the K of cdh_set_folds");
    return CDH_OK;
}

int32_t cv_write_fold_weights(cdh_handle h, int32_t k) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(kCvMaxGrid, (h->n + 255) / 256));
    CHK(dispatch(h, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        hipLaunchKernelGGL((k_fold_weights<T>), dim3(grid), dim3(256), 0, h->stream, (T*)h->w,
                           k >= 0 ? (const uint8_t*)h->cv.fold : (const uint8_t*)nullptr, h->n, (int)k);
        return CDH_OK;
    }));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CDH_OK;
}

// Host cost of a call, beside the launches: the packed image of B is rebuilt from the caller's B and uploaded whole, padding
// included -- O(srows * mpad) doubles through a pageable buffer, 32 MB at the limits (s = 4096, m = 1024) -- and the 0-based
// coordinate list and the summed record are fresh vectors too.  Small against the pass at the shapes cvLassoPath sends (a
// union support of tens of columns, a hundred lambdas: tens of KB), but part of any whole-call time that is quoted.
int32_t cv_path_sse(cdh_handle h, int32_t k, int64_t s, const int64_t* idx1, int64_t m, const double* B, int64_t ldb,
                    double* out_held, double* out_train) {
    CHK(cv_refuse_shards(h));
    const CvPlan pl = cv_plan(h->n, s, m);
    if (pl.refused) return fail(h, CDH_BAD_ARG, pl.refused);
    NEED_P(h, idx1);
    NEED_P(h, B);
    if (!out_held && !out_train) return fail(h, CDH_BAD_ARG, "out_held and out_train are both NULL");
    if (ldb < s) return fail(h, CDH_BAD_ARG, "need ldb >= s");
    if (!h->y_set) return fail(h, CDH_BAD_ARG, "cdh_path_sse needs y: call cdh_set_y first");
    if (k < -1) return fail(h, CDH_BAD_ARG, "k must be a fold, or -1 for none");
    if (k >= 0 && h->cv.K == 0) return fail(h, CDH_BAD_ARG, "k >= 0 needs cdh_set_folds first");
    if (k >= 0 && k >= h->cv.K) return fail(h, CDH_BAD_ARG, "k must be below the K of cdh_set_folds");
    for (int64_t t = 0; t < s; ++t)
        if (idx1[t] < 1 || idx1[t] > h->p) return fail(h, CDH_BAD_ARG, "idx1: coordinate out of range");
    HIPCHK(h, hipSetDevice(h->device));
    CHK(cv_scratch(h, pl.b_doubles));
    CvState& cv = h->cv;
    std::vector<int64_t> idx0((size_t)s);
    for (int64_t t = 0; t < s; ++t) idx0[(size_t)t] = idx1[t] - 1;
    std::vector<double> Bp((size_t)pl.b_doubles, 0.0);
    for (int64_t j = 0; j < m; ++j)
        for (int64_t t = 0; t < s; ++t) Bp[(size_t)cv_b_index(pl.srows, t, j)] = B[t + j * ldb];
    HIPCHK(h, hipMemcpyAsync(cv.idx, idx0.data(), sizeof(int64_t) * (size_t)s, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(cv.B, Bp.data(), sizeof(double) * (size_t)pl.b_doubles, hipMemcpyHostToDevice, h->stream));
    CHK(dispatch(h, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        for (int64_t g = 0; g < pl.groups; ++g)
            hipLaunchKernelGGL((k_path_sse<T>), dim3((unsigned)pl.grid), dim3(kCvRows), 0, h->stream, (const T*)h->X, h->ld, h->n,
                               (const T*)h->y, k >= 0 ? (const uint8_t*)cv.fold : (const uint8_t*)nullptr, (int)k,
                               (const int64_t*)cv.idx, (int)s, (int)pl.srows, (const double*)cv.B + g * pl.srows * kCvGroup,
                               (double*)cv.partials, (int)pl.nvals, (int)pl.mpad, (int)cv_group_first(g));
        return CDH_OK;
    }));
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)((pl.nvals + kReduceVals - 1) / kReduceVals)), dim3(64 * kReduceWaves), 0,
                       h->stream, (const double*)cv.partials, (int)pl.grid, (int)pl.nvals, (double*)cv.out);
    HIPCHK(h, hipGetLastError());
    std::vector<double> rec((size_t)pl.nvals);
    HIPCHK(h, hipMemcpyAsync(rec.data(), cv.out, sizeof(double) * (size_t)pl.nvals, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t j = 0; j < m; ++j) {
        if (out_held) out_held[j] = rec[(size_t)j];
        if (out_train) out_train[j] = rec[(size_t)(pl.mpad + j)];
    }
    return CDH_OK;
}
