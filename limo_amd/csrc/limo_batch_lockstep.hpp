// limo_batch_lockstep.hpp — the lock-step solve of a batch (LockStep: the Executor behind run_schedule, all windows advance together
// with one launch train per LM iteration) and the landmark-sharded exchange it calls between the kernels (ShardExchange).
// Part of limo_batch.hpp.
#pragma once

// =============================================================================================== LockStep
// Pinned flags, device lists of a re-batched active set and the full worklists (upload, behind the batch's pinned block).
inline int LockStep::alloc() {
    limo_ctx* ctx = b.ctx;
    const PackedBatch& P = b.P;
    h_flags_bytes = sizeof(int32_t) * std::max(1, P.n_win);
    HIP_TRY(ctx, ctx->host_alloc((void**)&h_flags, h_flags_bytes));
    if (b.dmalloc((void**)&d_act_blk, sizeof(int32_t) * std::max(1, P.n_blk))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_act_lblk, sizeof(int32_t) * std::max(1, P.n_lblk))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_act_sblk, sizeof(int32_t) * std::max(1, P.n_sblk))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_act_win, sizeof(int32_t) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_flags, sizeof(int32_t) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
    // full lists: a shard's are its own workgroups (Schur blocks: span 1), built here; an unsharded batch needs none but the
    // Schur list, which waits for its first lock-step solve (full_lists)
    wl.assign(b.pv.size(), ViewLists());
    for (size_t i = 0; i < wl.size(); ++i) {
        WorkLists& f = wl[i].full;
        f.n_blk = P.n_blk;
        f.n_lblk = P.n_lblk;
        f.n_win = P.n_win;
        if (b.shards.n_shards == 1) continue;
        const int r = wl[i].owner = b.shards.local[i];
        auto owned = [&](const std::vector<int32_t>& owner, const int32_t** list, int* n) -> int {
            std::vector<int32_t> v;
            for (size_t k = 0; k < owner.size(); ++k)
                if (owner[k] == r) v.push_back((int32_t)k);
            *n = (int)v.size();
            return upload_list(v, list);
        };
        if (owned(P.blk_owner, &f.blk, &f.n_blk) || owned(P.lblk_owner, &f.lblk, &f.n_lblk) || build_full_sblk(i)) return LIMO_ERR_RUNTIME;
    }
    return LIMO_OK;
}
inline int LockStep::create_events() {
    for (auto& e : act_ev) HIP_TRY(b.ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return LIMO_OK;
}
inline void LockStep::release_pinned() {
    if (h_flags) b.ctx->host_free(h_flags, h_flags_bytes);
}
inline void LockStep::destroy_events() {
    for (auto& e : act_ev)
        if (e) (void)hipEventDestroy(e);
}

// A worklist as a device block of this batch (a synchronous copy).
inline int LockStep::upload_list(const std::vector<int32_t>& v, const int32_t** out) {
    int32_t* d = nullptr;
    if (b.dmalloc((void**)&d, sizeof(int32_t) * std::max<size_t>(1, v.size()))) return LIMO_ERR_RUNTIME;
    if (!v.empty()) HIP_TRY(b.ctx, hipMemcpy(d, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice));
    *out = d;
    return LIMO_OK;
}
// The Schur worklist of every window, for producer view i.
inline int LockStep::build_full_sblk(size_t i) {
    WorkLists& f = wl[i].full;
    std::vector<int32_t> v;
    build_sblk_list(b.P, nullptr, b.c.schur_span, b.c.schur_span_gp, wl[i].owner, v, f.n_sblk_plain, f.n_sblk_fgp);
    f.n_sblk = (int)v.size();
    return upload_list(v, &f.sblk);
}

inline void LockStep::full_lists() {
    for (size_t i = 0; i < wl.size(); ++i) {
        if (!wl[i].full.sblk && build_full_sblk(i) != LIMO_OK && b.rc == LIMO_OK) b.rc = LIMO_ERR_RUNTIME;
        wl[i].cur = wl[i].full;
    }
}

// Rebuild the worklists from the windows that are active right now (synchronises the stream).  Unsharded batches only: a sharded
// batch has one window (batch_create_impl), and active_count() asks for eight.
inline void LockStep::rebatch() {
    if (b.shards.n_shards > 1) return;
    const PackedBatch& P = b.P;
    hipStream_t s = b.ctx->stream;
    hipLaunchKernelGGL(k_export_active, dim3(cdiv(P.n_win, 256)), dim3(256), 0, s, b.bv, d_flags);
    b.note(hipMemcpyAsync(h_flags, d_flags, sizeof(int32_t) * P.n_win, hipMemcpyDeviceToHost, s), "memcpy flags");
    b.note(hipStreamSynchronize(s), "sync flags");
    if (b.rc != LIMO_OK) return;
    std::vector<int32_t> wb, wlb, wsb, ww;
    for (int w = 0; w < P.n_win; ++w) {
        if (!h_flags[w]) continue;
        const WinDesc& d = P.win[w];
        ww.push_back(w);
        for (int i = 0; i < d.n_blk; ++i) wb.push_back(d.blk0 + i);
        for (int i = 0; i < d.n_lblk; ++i) wlb.push_back(d.lblk0 + i);
    }
    WorkLists& a = wl[0].cur;
    build_sblk_list(P, &ww, b.c.schur_span, b.c.schur_span_gp, -1, wsb, a.n_sblk_plain, a.n_sblk_fgp);
    auto up = [&](int32_t* dst, const std::vector<int32_t>& v, const int32_t*& list, int& n) {
        if (!v.empty()) b.note(hipMemcpyAsync(dst, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice, s), "upload worklist");
        list = dst;
        n = (int)v.size();
    };
    up(d_act_blk, wb, a.blk, a.n_blk);
    up(d_act_lblk, wlb, a.lblk, a.n_lblk);
    up(d_act_sblk, wsb, a.sblk, a.n_sblk);
    up(d_act_win, ww, a.win, a.n_win);
    b.note(hipStreamSynchronize(s), "sync worklists");  // the host vectors go out of scope
}

inline void LockStep::solve_init(int max_iter, int select) {
    it_no = 0;
    first_lin = true;  // the next linearisation defines the Jacobi scaling (WinState::compute_scale)
    assemble_pending = false;  // (a solve that ended right behind a linearisation leaves nothing for the next one)
    full_lists();
    hipLaunchKernelGGL(k_solve_init, dim3(cdiv(b.P.n_win, 256)), dim3(256), 0, b.ctx->stream, b.bv, b.c, max_iter, select);
    b.launch_check("k_solve_init");
}

inline void LockStep::linearize() {
    hipStream_t s = b.ctx->stream;
    if (b.P.TV) {
        hipLaunchKernelGGL(k_view_consts, dim3(cdiv(b.P.TV, 256)), dim3(256), 0, s, b.bv);
        b.launch_check("k_view_consts");
    }
    // ground-plane rows first: the landmark pass adds them to the landmark blocks
    EventPair* ep = b.timers.timed(LIMO_KERNEL_LINEARIZE);
    for (size_t i = 0; i < b.pv.size(); ++i)
        if (wl[i].cur.n_lblk) {
            b.launch_lin_lm(wl[i].cur.n_lblk, s, b.pv[i], wl[i].cur.lblk);
            b.launch_check("k_lin_lm");
        }
    b.timers.stop(ep, s);
    b.shards.reduce(0, wl[0].cur.win, wl[0].cur.n_win);
    // Sharded: the camera assembly only has to come before the Schur complement when it defines the Jacobi scale (the
    // first linearisation of a solve).  Every other iteration it waits for the slabs and ONE exchange serves both (step()).
    if (b.shards.n_shards > 1 && !first_lin) {
        assemble_pending = true;
        return;
    }
    first_lin = false;
    b.shards.exchange(1);
    assemble(it_no);
}

// k_cam_assemble + the active-window counter of iteration `iter`: a ring of 4 slots so the host can read iteration i-1
// while iteration i runs
inline void LockStep::assemble(int iter) {
    hipStream_t s = b.ctx->stream;
    const int slot = iter & 3;
    BatchView bvs = b.bv;
    bvs.n_active = b.bv.n_active + 2 * slot;
    bvs.n_active_host = b.d_pin->active + slot;
    const WorkLists& a = wl[0].cur;
    b.launch_cam_assemble(bvs, a.win, a.n_win, s);
    b.launch_check("k_cam_assemble");
    b.note(hipEventRecord(act_ev[slot], s), "record n_active");
}

// Lagging by one iteration: the count of iteration i-1 is read while iteration i is already enqueued, so the
// host never drains the stream inside a solve.  The price is at most one extra iteration of no-op launches.
inline int LockStep::active_count() {
    if (b.rc != LIMO_OK) return 0;
    const int cur = it_no++;
    if (cur == 0) return b.P.n_win;  // iteration zero: nothing to wait for yet
    const int slot = (cur - 1) & 3;
    b.note(hipEventSynchronize(act_ev[slot]), "sync n_active");
    if (b.rc != LIMO_OK) return 0;
    const int a = b.h_pin->active[slot], listed = wl[0].cur.n_win;
    static const bool trace = std::getenv("KBA_TRACE_ACTIVE") != nullptr;  // profiling aid
    if (trace) std::fprintf(stderr, "[kba] iteration %d: active %d, listed %d, span %d\n", cur - 1, a, listed, b.c.schur_span);
    // re-batch when at most half of the listed windows still iterate (and the list is worth shrinking)
    if (a > 0 && listed >= 8 && 2 * a <= listed) rebatch();
    return a;
}

inline void LockStep::expire(int) {
    if (assemble_pending) {  // sharded: the camera assembly of the last linearisation was deferred behind the Schur slabs - the
                             // time cap ends the solve before them: assemble now (exchange of the linearisation sums only), so
                             // that the windows' cost is the cost of the point they stop at
        assemble_pending = false;
        b.shards.exchange(1);
        assemble(it_no - 1);
    }
    hipLaunchKernelGGL(k_expire, dim3(cdiv(b.P.n_win, 256)), dim3(256), 0, b.ctx->stream, b.bv);
    b.launch_check("k_expire");
}

inline void LockStep::step() {
    hipStream_t s = b.ctx->stream;
    const std::vector<BatchView>& pv = b.pv;
    if (b.c.slab_packed) b.spart_has_packed = true;
    const WorkLists& a = wl[0].cur;  // (the window list is the same for every view)
    {
        // (a step without Schur blocks - no window with a variable landmark - launches nothing and counts no launch)
        int n_schur = 0;
        for (size_t i = 0; i < pv.size(); ++i) n_schur += wl[i].cur.n_sblk;
        EventPair* ep = n_schur ? b.timers.timed(LIMO_KERNEL_SCHUR) : nullptr;
        for (size_t i = 0; i < pv.size(); ++i) {
            const WorkLists& l = wl[i].cur;
            b.launch_schur(pv[i], l.sblk, l.n_sblk_plain, l.sblk + l.n_sblk_plain, l.n_sblk_fgp, l.sblk + l.n_sblk_plain + l.n_sblk_fgp,
                           l.n_sblk - l.n_sblk_plain - l.n_sblk_fgp, false, s);
            b.launch_check("Schur kernels");
        }
        b.timers.stop(ep, s);
    }
    b.shards.reduce(1, a.win, a.n_win);
    if (assemble_pending) {  // sharded, ONE exchange: camera-side sums + ground-plane blocks + scalars + [S | rhs]
        assemble_pending = false;
        b.shards.exchange(3);
        assemble(it_no - 1);  // (active_count() has moved it_no on to the next iteration)
    } else {
        b.shards.exchange(2);
    }
    b.launch_cam_solve(b.bv, a.win, a.n_win, s);
    b.launch_check("k_cam_solve");
    for (size_t i = 0; i < pv.size(); ++i) {
        b.launch_backsub(pv[i], wl[i].cur.lblk, wl[i].cur.n_lblk, s);
        b.launch_check("k_backsub");
    }
    b.shards.reduce(2, a.win, a.n_win);
    b.shards.exchange(4);
    b.launch_step_decide(b.bv, a.win, a.n_win, s);
    b.launch_check("k_step_decide");
    for (size_t i = 0; i < pv.size(); ++i) {  // a rejected step: its landmark blocks are damped again for the next iteration
        b.launch_after_step(pv[i], wl[i].cur.lblk, wl[i].cur.n_lblk, s);
        b.launch_check("k_after_step");
    }
}

inline void LockStep::trim() {
    hipStream_t s = b.ctx->stream;
    const std::vector<BatchView>& pv = b.pv;
    bool any = false;
    for (const WinDesc& d : b.P.win) any = any || d.do_trim;
    if (!any) return;
    for (size_t i = 0; i < pv.size(); ++i) {
        b.launch_trim_residual(pv[i], wl[i].full.blk, wl[i].full.n_blk, s);
        b.launch_check("k_trim_residual");
    }
    for (size_t i = 0; i < pv.size(); ++i) {
        b.launch_trim_max(pv[i], b.shards.local[i], cdiv(b.P.TL, kBlock), s);
        b.launch_check("k_trim_max");
    }
    b.shards.exchange_trim();
    b.launch_trim_select(b.bv, b.P.n_win, s);
    b.launch_check("k_trim_select");
}

// =============================================================================================== ShardExchange
// The sharded half of upload: producer views with their blocks, the consumer view's arena and window descriptors.
inline int ShardExchange::setup() {
    if (n_shards == 1) return LIMO_OK;
    limo_ctx* ctx = b.ctx;
    xl = exchange_layout(b.P);
    d_win_orig = const_cast<WinDesc*>(b.bv.win);
    b.pv.assign(local.size(), b.bv);  // producers keep the batch's own per-workgroup arrays (every entry has ONE owner)
    auto zeros = [&](double** out, size_t n) -> int {
        if (b.dmalloc((void**)out, sizeof(double) * std::max<size_t>(1, n))) return LIMO_ERR_RUNTIME;
        HIP_TRY(ctx, hipMemsetAsync(*out, 0, sizeof(double) * std::max<size_t>(1, n), ctx->stream));
        return LIMO_OK;
    };
    if (zeros(&arena_c, xl.c_total)) return LIMO_ERR_RUNTIME;
    trims.assign(1 + local.size(), nullptr);
    for (double*& t : trims)
        if (zeros(&t, xl.trim_count)) return LIMO_ERR_RUNTIME;
    blocks.assign(local.size(), nullptr);
    if (!is_virtual && zeros(&d_gather, (size_t)ctx->comm_world * xl.b_total)) return LIMO_ERR_RUNTIME;
    {   // consumer view: "P workgroups, P rows" per window
        std::vector<WinDesc> wc = exchange_consumer_windows(b.P);
        WinDesc* d_wc = nullptr;
        if (b.dmalloc((void**)&d_wc, sizeof(WinDesc) * wc.size())) return LIMO_ERR_RUNTIME;
        HIP_TRY(ctx, hipMemcpy(d_wc, wc.data(), sizeof(WinDesc) * wc.size(), hipMemcpyHostToDevice));
        exchange_bind_consumer(xl, b.bv, arena_c, trims[0], d_wc);
    }
    for (size_t i = 0; i < local.size(); ++i) {
        if (zeros(&blocks[i], xl.b_total)) return LIMO_ERR_RUNTIME;  // the shard's own block ...
        exchange_bind_producer(xl, b.pv[i], blocks[i], trims[1 + i]);
        if (zeros(&b.pv[i].S_part, xl.spart_count)) return LIMO_ERR_RUNTIME;  // ... and its private Schur slabs
    }
    if (!is_virtual && b.dmalloc((void**)&d_lm_tmp, sizeof(double) * 3 * std::max(1, b.P.TL))) return LIMO_ERR_RUNTIME;
    return LIMO_OK;
}

// Every local shard's partial sums into its block, over the listed windows.  what = 0: the linearisation sums; 1: the Schur
// right-hand sides, and the tile slabs of the shard summed; 2: the back-substitution's scalars.
inline void ShardExchange::reduce(int what, const int32_t* win, int n_win) {
    if (n_shards == 1 || !n_win) return;
    hipStream_t s = b.ctx->stream;
    for (size_t i = 0; i < b.pv.size(); ++i) {
        hipLaunchKernelGGL(k_shard_reduce, dim3(n_win), dim3(kBlock), 0, s, b.pv[i], win, local[i], what);
        if (what == 1) hipLaunchKernelGGL(k_slab_reduce, dim3(n_win, 8), dim3(kBlock), 0, s, b.pv[i], win, n_shards);
        b.launch_check(what == 1 ? "k_slab_reduce" : "k_shard_reduce");
    }
}

// Per-iteration exchange (point 1 = A1, 2 = A2, 3 = A, 4 = B; kba_buffers.hpp:exchange_layout): ALL-GATHER of the shards'
// blocks over the ranks - one call per local slot, normally one shard per rank: ONE ncclAllGather of 41 KB at a C4 window -
// then k_unpack puts every contribution at its shard's place in the consumer view.  Shard s lives on rank s mod world, in
// local slot s / world.  Virtual shards (no communicator): the unpack alone.
inline void ShardExchange::exchange(int point) {
    if (n_shards == 1) return;
    limo_ctx* ctx = b.ctx;
    hipStream_t s = ctx->stream;
    size_t off, count;
    xl.range(point, off, count);
    for (size_t i = 0; i < b.pv.size(); ++i) {
        if (is_virtual) {
            hipLaunchKernelGGL(k_unpack, dim3(cdiv((int64_t)count, 256)), dim3(256), 0, s, xl, (const WinDesc*)d_win_orig, (const double*)(blocks[i] + off), arena_c,
                               local[i], (int64_t)off, (int64_t)count);
            b.launch_check("k_unpack");
        } else {
            if (ctx->xfn) {
                host_exchange(blocks[i] + off, d_gather, count, 0);
            } else {
                b.note_nccl(ncclAllGather(blocks[i] + off, d_gather, count, ncclDouble, (ncclComm_t)ctx->comm, s), "ncclAllGather");
            }
            for (int q = 0; q < ctx->comm_world; ++q) {
                hipLaunchKernelGGL(k_unpack, dim3(cdiv((int64_t)count, 256)), dim3(256), 0, s, xl, (const WinDesc*)d_win_orig,
                                   (const double*)(d_gather + (size_t)q * count), arena_c, (int)i * ctx->comm_world + q, (int64_t)off, (int64_t)count);
                b.launch_check("k_unpack");
            }
        }
        ++n_exchanges;
        exchange_bytes += (int64_t)count * (int64_t)sizeof(double);
    }
}
// The caller's transport (limo_ctx_comm_init_host): `count` doubles at `src` (device) go to the host, through the callback
// (kind 0: all-gather into world * count doubles, rank order; kind 1: sum over the ranks into count doubles) and back to `dst`.
inline void ShardExchange::host_exchange(const double* src, double* dst, size_t count, int kind) {
    limo_ctx* ctx = b.ctx;
    hipStream_t s = ctx->stream;
    const size_t n_out = kind == 0 ? (size_t)ctx->comm_world * count : count, need = count + n_out;
    if (ctx->xhost.ensure(sizeof(double) * need) != hipSuccess) {
        b.note(hipErrorOutOfMemory, "hipHostMalloc(exchange staging)");
        std::vector<double> z(need, 0.0);  // (the peers are still met: see below)
        ctx->xfn(z.data(), z.data() + count, (long long)count, kind, ctx->xuser);
        return;
    }
    double* const xhost = static_cast<double*>(ctx->xhost.p);
    // The transport is a COLLECTIVE: a rank that skipped it after a local error would leave its peers blocked in it for ever.  So
    // the call is made in every case - after an error with a zeroed contribution - and only the device copies are skipped; the
    // solve of this rank ends with LIMO_ERR_RUNTIME, the peers' solves end (with a result that misses this rank's share).
    if (b.rc == LIMO_OK) {
        b.note(hipMemcpyAsync(xhost, src, sizeof(double) * count, hipMemcpyDeviceToHost, s), "exchange: device -> host");
        b.note(hipStreamSynchronize(s), "exchange: sync");
    }
    if (b.rc != LIMO_OK) std::memset(xhost, 0, sizeof(double) * count);
    ctx->xfn(xhost, xhost + count, (long long)count, kind, ctx->xuser);
    if (b.rc != LIMO_OK) return;
    b.note(hipMemcpyAsync(dst, xhost + count, sizeof(double) * n_out, hipMemcpyHostToDevice, s), "exchange: host -> device");
    b.note(hipStreamSynchronize(s), "exchange: sync");  // (the staging buffer is reused by the next step)
}
// Trimming round: per-landmark residual maxima, one owner per entry and zero elsewhere - an exact sum in any order.
inline void ShardExchange::exchange_trim() {
    if (n_shards == 1) return;
    limo_ctx* ctx = b.ctx;
    hipStream_t s = ctx->stream;
    const int64_t n = (int64_t)xl.trim_count;
    ShardPtrs sp;
    for (size_t i = 0; i < b.pv.size(); ++i) sp.p[i] = trims[1 + i];
    hipLaunchKernelGGL(k_sum_shards<double>, dim3(cdiv(n, 256)), dim3(256), 0, s, trims[0], sp, (int)b.pv.size(), n);
    b.launch_check("k_sum_shards");
    if (!is_virtual && ctx->xfn) {
        host_exchange(trims[0], trims[0], (size_t)n, 1);
    } else if (!is_virtual) {
        b.note_nccl(ncclAllReduce(trims[0], trims[0], (size_t)n, ncclDouble, ncclSum, (ncclComm_t)ctx->comm, s), "ncclAllReduce");
    }
    ++n_exchanges;
    exchange_bytes += n * (int64_t)sizeof(double);
}
// The end of a solve whose shards are ranks: every rank ends with every landmark - the sum of "owned, else zero".
inline int ShardExchange::gather_landmarks() {
    if (n_shards == 1 || is_virtual) return LIMO_OK;
    limo_ctx* ctx = b.ctx;
    hipLaunchKernelGGL(k_lm_owned, dim3(cdiv(b.P.TL, 256)), dim3(256), 0, ctx->stream, b.bv, d_lm_tmp, rank, n_shards, ctx->comm_world);
    if (ctx->xfn) {
        host_exchange(d_lm_tmp, b.bv.lm, (size_t)3 * b.P.TL, 1);
        if (b.rc != LIMO_OK) return b.rc;
    } else {
        const ncclResult_t r = ncclAllReduce(d_lm_tmp, b.bv.lm, (size_t)3 * b.P.TL, ncclDouble, ncclSum, (ncclComm_t)ctx->comm, ctx->stream);
        b.note_nccl(r, "ncclAllReduce(landmarks)");
        if (r != ncclSuccess) return b.rc;
    }
    ++n_exchanges;
    exchange_bytes += (int64_t)sizeof(double) * 3 * b.P.TL;
    return LIMO_OK;
}
