// sweep.hpp -- the streamed sweep: one chunk of a pass enqueued as launches of the step kernels (run_chunk and its three
// launchers, captured and replayed as a graph where that pays).  Included by cdhip.hip, in its anonymous namespace.  What a
// launch looks like -- grids, the k_gramstep variant, chunk lengths, the graph key, the profile's byte model -- is
// sweep_plan.hpp's to say: nothing here derives a number.

// does any coordinate repeat in the chunk?  (scheduler-made lists never do; caller-made ones may)
void note_duplicates(cdh_handle h, const int64_t* idx0, int m) {
    if ((int64_t)h->stamp.size() != h->p) h->stamp.assign((size_t)h->p, 0);
    h->chunk_dup = false;
    for (int i = 0; i < m; ++i) {
        if (h->stamp[(size_t)idx0[i]]) { h->chunk_dup = true; break; }
        h->stamp[(size_t)idx0[i]] = 1;
    }
    for (int i = 0; i < m; ++i) h->stamp[(size_t)idx0[i]] = 0;
}

// The visits of a chunk have been enqueued (streamed, or in covariance form): bring their results back,
// replay them on the host-side SparseIterate, and tell the gradient cache what moved.
int32_t finish_chunk(cdh_handle h, const int64_t* idx0, int m, double* maxH) {
    HIPCHK(h, hipMemcpyAsync(h->h_hs, h->d_hs, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_newval, h->d_newval, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_touched, h->d_touched, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_ctrl, h->d_ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    CHK(p2p_check(h));
    if (h->h_ctrl->domain_error) h->domain_error = true;
    const double mh = h->h_ctrl->maxH;
    if (mh > *maxH) *maxH = mh;   // a NaN h never raises maxH: `abs(h) > maxH` (coordinate_descent.jl:104)
    // replay the SparseIterate writes of the visits in order (x[k] += b/a ; cdprox!)
    for (int i = 0; i < m; ++i) {
        const int64_t k = idx0[i];
        if (h->h_touched[i] && h->x.get(k) == 0.0) h->x.set(k, 1.0);  // pre-prox non-zero: slot appended
        h->x.set(k, h->h_newval[i]);
    }
    gc_note_moves(h, idx0, m);
    return CDH_OK;
}

// ---- one chunk of a pass: visits idx0[0..m) -------------------------------------------
// Each launcher: per block of visits the step kernel, then the record's reduction -- finalised on the spot, or (row shards) summed
// over the ranks first and finalised by the scalar stage -- and after the last block the axpy of its moves.
template <typename T, int B> int32_t launch_block_chunk(cdh_handle h, int m) {
    constexpr int NREC = BlockRec<B>::N;
    const int G = h->sz.block_grid;
    int nprev = 0;
    for (int pos0 = 0; pos0 < m; pos0 += B) {
        const int nb = std::min(B, m - pos0);
        hipLaunchKernelGGL((k_blockstep<T, B>), dim3(G), dim3(kBlock), 0, h->stream, (const T*)h->X,
                           h->ld, h->nvec, (T*)h->r, h->d_idx, h->d_hs, pos0, nb, nprev, h->d_partials);
        auto finalize = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(1), dim3(1024), 0, h->stream, h->d_partials, G, nb, h->d_ctrl, h->beta, h->omega,
                               h->d_idx, h->d_hs, h->d_newval, h->d_touched, pos0, h->d_red);
        };
        if (!h->xs.sharded()) {
            finalize(k_block_finalize<B, true>);
        } else {
            finalize(k_block_finalize<B, false>);
            CHK(allreduce(h, h->d_red, NREC));
            hipLaunchKernelGGL((k_block_scalar<B>), dim3(1), dim3(64), 0, h->stream, h->d_red, nb,
                               h->d_ctrl, h->beta, h->omega, h->d_idx, h->d_hs, h->d_newval,
                               h->d_touched, pos0);
        }
        nprev = nb;
    }
    const int last0 = ((m - 1) / B) * B;
    hipLaunchKernelGGL((k_block_axpy<T, B>), dim3(G), dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld,
                       h->nvec, (T*)h->r, h->d_idx, h->d_hs, last0, m - last0);
    return CDH_OK;
}

// wide blocks (B = 16 / 32 / 64): MFMA-accumulated Gram kernel + two-stage reduction
template <typename T, int NG> int32_t launch_gram_chunk(cdh_handle h, int m) {
    using R = GramRec<NG>;
    constexpr int B = R::B;
    const T* wts = h->has_w ? (const T*)h->w : (const T*)nullptr;
    const GramPlan pl = gram_plan(h->nvec, h->n, h->sz.cus, NG, (int)sizeof(T), h->knobs.lt, h->knobs.ks);
    const int G = pl.grid;
    CHK(need_partials(h, (size_t)G * R::N, "partial buffer too small for this grid"));
    int nprev = 0;
    for (int pos0 = 0; pos0 < m; pos0 += B) {
        const int nb = std::min(B, m - pos0);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(G), dim3(64 * kGramWaves), 0, h->stream, (const T*)h->X, h->ld, h->nvec,
                               wts, (T*)h->r, h->d_idx, h->d_hs, pos0, nb, nprev, h->d_partials);
        };
        // (the plan keeps fp32 B = 64 on the fragment path: its LDS-transposed variants are not instantiated)
        constexpr bool kHasLt = !(NG == 4 && sizeof(T) == 4);
        switch (pl.variant) {
        case kGramLtShort: if constexpr (kHasLt) go(k_gramstep<T, NG, true, 1>); break;
        case kGramLtLong: if constexpr (kHasLt) go(k_gramstep<T, NG, true>); break;
        case kGramFrag: go(k_gramstep<T, NG>); break;
        }
        hipLaunchKernelGGL(k_gram_reduce, dim3((R::N + kReduceVals - 1) / kReduceVals), dim3(64 * kReduceWaves), 0, h->stream, h->d_partials, G, R::N, h->d_red);
        CHK(allreduce(h, h->d_red, R::N));
        hipLaunchKernelGGL((k_gram_scalar<NG>), dim3(1), dim3(64), 0, h->stream, h->d_red, nb, h->chunk_dup ? 1 : 0, h->d_ctrl,
                           h->beta, h->omega, h->d_idx, h->d_hs, h->d_newval, h->d_touched, pos0);
        nprev = nb;
    }
    const int last0 = ((m - 1) / B) * B;
    hipLaunchKernelGGL(k_multi_axpy<T>, dim3(h->sz.step_grid), dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld,
                       h->nvec, (T*)h->r, h->d_idx, h->d_hs, last0, m - last0);
    return CDH_OK;
}

template <typename T> int32_t launch_coord_chunk(cdh_handle h, int m) {
    const int G = h->sz.step_grid;
    for (int pos = 0; pos < m; ++pos) {
        auto step = [&](auto kernel, const T* wts) {
            hipLaunchKernelGGL(kernel, dim3(G), dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld, h->nvec, wts, (T*)h->r,
                               h->d_idx, h->d_hs, pos, h->d_partials);
        };
        if (h->has_w) step(k_step<T, true>, (const T*)h->w); else step(k_step<T, false>, (const T*)nullptr);
        auto finalize = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(1), dim3(kBlock), 0, h->stream, h->d_partials, G, h->d_ctrl, h->beta, h->omega,
                               h->d_idx, h->d_hs, h->d_newval, h->d_touched, pos, h->d_red);
        };
        if (!h->xs.sharded()) {
            finalize(k_finalize<true>);
        } else {
            finalize(k_finalize<false>);
            CHK(allreduce(h, h->d_red, 4));
            hipLaunchKernelGGL(k_scalar_update, dim3(1), dim3(64), 0, h->stream, h->d_red, h->d_ctrl,
                               h->beta, h->omega, h->d_idx, h->d_hs, h->d_newval, h->d_touched, pos);
        }
    }
    hipLaunchKernelGGL(k_axpy<T>, dim3(G), dim3(kBlock), 0, h->stream, (const T*)h->X, h->ld, h->nvec,
                       (T*)h->r, h->d_idx, h->d_hs, m);
    return CDH_OK;
}

int32_t all_ranks_agree(cdh_handle h, bool mine, bool* all);   // grad_cache.hpp
int32_t agree_default_width(cdh_handle h) {
    if (h->width_agreed || !h->width_default || !h->xs.sharded() || h->xs.nranks() <= 1) return CDH_OK;
    bool all64 = false;
    CHK(all_ranks_agree(h, h->blockB == 64, &all64));
    if (!all64) h->blockB = 32;      // some shard is on the long side of the cut: every rank takes the long-column width
    h->width_agreed = true;
    return CDH_OK;
}

int32_t run_chunk(cdh_handle h, const int64_t* idx0, int m, double* maxH) {
    CHK(agree_default_width(h));
    CHK(sync_r(h));   // the streaming kernels read and write r
    h->rs.stream_begins();
    h->xs.chunk_begins();
    std::memcpy(h->h_idx, idx0, sizeof(int64_t) * (size_t)m);
    note_duplicates(h, idx0, m);
    HIPCHK(h, hipMemcpyAsync(h->d_idx, h->h_idx, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, h->stream));
    h->ctrl.maxH = 0.0;
    h->ctrl.domain_error = 0;
    CHK(upload_ctrl(h));
    HIPCHK(h, h->prof.begin(h->stream));
    const ChunkRoute route = chunk_route(h->mode == CDH_SWEEP_BLOCK, h->blockB, h->has_w, m, h->xs.graph_key_bits(), h->chunk_dup);
    auto enqueue = [&]() {
        return dispatch(h, [&](auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            if (!route.blocked) return launch_coord_chunk<T>(h, m);
            if (h->blockB == 64) return launch_gram_chunk<T, 4>(h, m);
            if (h->blockB == 32) return launch_gram_chunk<T, 2>(h, m);
            if (h->blockB == 16) return launch_gram_chunk<T, 1>(h, m);
            if (h->blockB == 8) return launch_block_chunk<T, 8>(h, m);
            if (h->blockB == 4) return launch_block_chunk<T, 4>(h, m);
            return launch_block_chunk<T, 2>(h, m);
        });
    };
    // hipGraph replay: the launch sequence of an m-visit chunk depends only on (m, mode, B, exchange) --
    // every kernel takes its visit position as a literal and reads idx / hs / lambda from device
    // memory -- so one captured graph serves every later pass of that length.  Row shards too: the
    // direct exchange reads its epoch base from device memory (set before each replay), RCCL
    // all-reduces are recorded by RCCL itself as graph nodes.  Only the host-staged exchange cannot
    // be recorded.  A failed capture switches the handle back to node-by-node launches for good.
    bool launched = false;
    if (h->use_graph && !h->graph_broken && h->xs.may_capture() && route.graph_worth) {
        const GraphEntry* entry = h->graphs.find(route.key);
        if (!entry) {
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            h->xs.capture_begins();
            hipError_t e0 = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
            const int32_t erc = e0 == hipSuccess ? enqueue() : (int32_t)CDH_HIP_ERROR;
            hipError_t e1 = e0 == hipSuccess ? hipStreamEndCapture(h->stream, &graph) : e0;
            const cdh::Captured holds = h->xs.capture_ends();
            if (erc == CDH_OK && e1 == hipSuccess && graph) e1 = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            if (graph) (void)hipGraphDestroy(graph);
            if (erc != CDH_OK || e1 != hipSuccess || !exec) {
                (void)hipGetLastError();
                h->graph_broken = true;
            } else {
                entry = h->graphs.insert({route.key, exec, holds});
            }
        }
        if (entry) {
            if (entry->holds.exchanges)   // they run under the epochs base + 1 .. base + exchanges
                hipLaunchKernelGGL(cdk::k_set_u32, dim3(1), dim3(1), 0, h->stream, h->d_p2p_base, h->xs.reserve_epochs(entry->holds.exchanges));
            h->xs.replay_counted(entry->holds);
            HIPCHK(h, hipGraphLaunch(entry->exec, h->stream));
            launched = true;
        }
    }
    if (!launched) CHK(enqueue());
    h->rs.stream_enqueued(route.rewrites);   // one rewrite of r per launch that applies updates
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->prof.stop(h->stream));
    CHK(finish_chunk(h, idx0, m, maxH));
    if (h->prof.on) {
        const ChunkTraffic t = chunk_traffic(route.blocked, h->blockB, m, h->has_w, h->h_hs, h->n, h->esz);
        HIPCHK(h, h->prof.end(t.launches, t.bytes));
    }
    return CDH_OK;
}
