// limo_batch_stream.hpp — the streaming solve of a batch (StreamSolve): the windows move through slots, the host enqueues rounds of
// the launch train over the slot groups' lists and learns from a pinned word that all windows are done.  Part of limo_batch.hpp.
#pragma once

inline void StreamSolve::teardown() {
    for (StreamGroup& g : groups) {
        if (g.own_stream && g.stream) (void)hipStreamDestroy(g.stream);
        if (g.trim_stream) (void)hipStreamDestroy(g.trim_stream);
        for (hipEvent_t e : {g.sched_ev, g.trim_ev, g.done_ev, g.round_ev[0], g.round_ev[1], g.round_ev[2], g.round_ev[3]})
            if (e) (void)hipEventDestroy(e);
        if (g.h_done) b.ctx->host_free(g.h_done, 64);
    }
    groups.clear();
    if (start_ev) (void)hipEventDestroy(start_ev);
    start_ev = nullptr;
}

// Streams, events, lists and scheduler state of the slot groups of `geo` (kba_batch_plan.hpp:stream_geometry), kept for the
// re-solves of the batch while the number of groups stays (the rest of the geometry is fixed by the batch).
inline int StreamSolve::setup(const StreamGeometry& geo) {
    limo_ctx* ctx = b.ctx;
    const int n_groups = geo.n_groups;
    if (groups_built == n_groups) return LIMO_OK;
    (void)hipStreamSynchronize(ctx->stream);
    teardown();  // (device blocks of an earlier layout stay with the batch until it is destroyed)
    n_slots = geo.n_slots;
    if (!d_sched_ctl && b.dmalloc((void**)&d_sched_ctl, sizeof(int32_t) * 8)) return LIMO_ERR_RUNTIME;
    HIP_TRY(ctx, hipEventCreateWithFlags(&start_ev, hipEventDisableTiming));
    groups.resize(n_groups);
    for (int gi = 0; gi < n_groups; ++gi) {
        StreamGroup& g = groups[gi];
        g.n_slots = geo.group_slots[gi];
        g.sv = b.bv;
        size_t total = 0;
        for (int k = 0; k < SL_COUNT; ++k) {
            g.mx[k] = geo.mx[k];
            g.cap[k] = g.n_slots * g.mx[k];
            g.sv.sched_off[k] = (int32_t)total;
            total += 1 + (size_t)std::max(1, g.cap[k]);
        }
        if (b.dmalloc((void**)&g.d_lists, sizeof(int32_t) * total)) return LIMO_ERR_RUNTIME;
        if (b.dmalloc((void**)&g.d_slot_win, sizeof(int32_t) * std::max(1, g.n_slots))) return LIMO_ERR_RUNTIME;
        if (b.dmalloc((void**)&g.d_slot_cnt, sizeof(int32_t) * (SL_COUNT + 1) * std::max(1, g.n_slots))) return LIMO_ERR_RUNTIME;
        HIP_TRY(ctx, hipMemsetAsync(g.d_lists, 0, sizeof(int32_t) * total, ctx->stream));
        HIP_TRY(ctx, ctx->host_alloc((void**)&g.h_done, 64));
        HIP_TRY(ctx, hipHostGetDevicePointer((void**)&g.d_h_done, g.h_done, 0));
        for (auto& e : g.round_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&g.sched_ev, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&g.trim_ev, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&g.done_ev, hipEventDisableTiming));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&g.trim_stream, hipStreamNonBlocking));
        if (gi == 0) {
            g.stream = nullptr;  // the context's stream, looked up at solve time (limo_ctx_set_stream)
        } else {
            HIP_TRY(ctx, hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
            g.own_stream = true;
        }
        g.sv.counted = 1;
        g.sv.n_slots = g.n_slots;
        g.sv.slot_win = g.d_slot_win;
        g.sv.sched_ctl = d_sched_ctl;
        g.sv.slot_cnt = g.d_slot_cnt;
        g.sv.sched_lists = g.d_lists;
        g.sv.sched_done_host = g.d_h_done;
        g.sv.n_active_host = nullptr;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    groups_built = n_groups;
    return LIMO_OK;
}

// One round of one group = scheduler + (side stream) trimming of the windows whose trimming solve just ended + one LM
// iteration of every window in the group's slots.  The launch train (round 6): the per-view constants inside k_sched_fill,
// accepted landmarks + re-damping in ONE launch (k_after_step) - 12 launches per round instead of 14.
// in_flight_max: an upper bound on the windows this group can have in its slots in this round (the batch's unfinished windows as
// of the pinned done-counter the host read last).  The list-driven kernels are launched over bound x (entries per window)
// workgroups instead of the lists' capacities: while the batch drains, a round of 200 windows in 2048 slots no longer
// dispatches 16 000 workgroups per kernel that read one count word and leave (~3 ns each: 50 us per kernel, and a round has
// a dozen of them - the "launch-latency floor" of the drain was mostly this).
inline void StreamSolve::enqueue_round(StreamGroup& g, int round, bool time_kernels, int in_flight_max) {
    hipStream_t s = g.stream;
    const BatchView& sv = g.sv;
    int cap[SL_COUNT];
    const int bound = std::max(1, std::min(g.n_slots, in_flight_max));
    for (int k = 0; k < SL_COUNT; ++k) cap[k] = std::min(g.cap[k], bound * g.mx[k]);
    auto L = [&](int k) { return (const int32_t*)(g.d_lists + sv.sched_off[k] + 1); };
    if (round > 0) b.note(hipStreamWaitEvent(s, g.trim_ev, 0), "wait trim");  // last round's trimming re-armed its windows
    hipLaunchKernelGGL(k_sched_advance, dim3(cdiv(g.n_slots, 256)), dim3(256), 0, s, sv, b.c);
    hipLaunchKernelGGL(k_sched_scan, dim3(1), dim3(kSchedThreads), 0, s, sv, round);
    hipLaunchKernelGGL(k_sched_fill, dim3(cdiv(g.n_slots, 4)), dim3(256), 0, s, sv, b.c);
    b.launch_check("scheduler kernels");
    // ---- trimming of the windows whose trimming solve just ended, on the side stream: k_trim_select is a
    //      latency-bound sort (one workgroup per window, ~0.3 ms) - the other windows iterate meanwhile, the
    //      trimmed ones join again in the next round (k_trim_select arms their next solve)
    b.note(hipEventRecord(g.sched_ev, s), "record sched");
    b.note(hipStreamWaitEvent(g.trim_stream, g.sched_ev, 0), "wait sched");
    b.launch_trim_residual(sv, L(SL_TBLK), cap[SL_TBLK], g.trim_stream);
    b.launch_trim_max(sv, 0, cap[SL_TLBLK], g.trim_stream);
    b.launch_trim_select(sv, cap[SL_TWIN], g.trim_stream);
    b.launch_check("trim kernels");
    b.note(hipEventRecord(g.trim_ev, g.trim_stream), "record trim");
    // ---- linearisation of the windows that need it (their per-view constants: k_sched_fill above)
    {
        EventPair* ep = time_kernels ? b.timers.timed(LIMO_KERNEL_LINEARIZE, s) : nullptr;
        if (cap[SL_LBLK]) b.launch_lin_lm(cap[SL_LBLK], s, sv, L(SL_LBLK));
        b.timers.stop(ep, s);
    }
    b.launch_cam_assemble(sv, L(SL_WIN), cap[SL_WIN], s);
    b.launch_check("linearisation kernels");
    // ---- trust-region step of the windows that iterate
    {
        EventPair* ep = time_kernels && (cap[SL_SPLAIN] || cap[SL_SFGP] || cap[SL_SGEN]) ? b.timers.timed(LIMO_KERNEL_SCHUR, s) : nullptr;
        // few windows in flight (the batch drains): both fast-class lists in one launch (kba_kernels.hip:k_schur_lean_pair)
        const bool pair = b.schur_pair_ok && bound <= kSchurPairBound && cap[SL_SPLAIN] && cap[SL_SFGP];
        b.launch_schur(sv, L(SL_SPLAIN), cap[SL_SPLAIN], L(SL_SFGP), cap[SL_SFGP], L(SL_SGEN), cap[SL_SGEN], pair, s);
        b.timers.stop(ep, s);
    }
    b.launch_cam_solve(sv, L(SL_WIN), cap[SL_WIN], s);
    b.launch_backsub(sv, L(SL_LBLK), cap[SL_LBLK], s);
    b.launch_step_decide(sv, L(SL_WIN), cap[SL_WIN], s);
    b.launch_after_step(sv, L(SL_LBLK), cap[SL_LBLK], s);
    b.launch_check("step kernels");
    b.note(hipEventRecord(g.round_ev[round & 3], s), "record round");
}

// The host only enqueues; it learns that all windows are done from a pinned word the scheduler writes, two rounds
// late (so the streams never drain inside a solve).
inline int StreamSolve::solve() {
    limo_ctx* ctx = b.ctx;
    const PackedBatch& P = b.P;
    if (setup(stream_geometry(P, {b.c.schur_span, b.c.schur_span_gp}, b.run.sw)) != LIMO_OK) return LIMO_ERR_RUNTIME;
    if (b.c.slab_packed) b.spart_has_packed = true;
    hipStream_t s0 = ctx->stream;
    groups[0].stream = s0;
    HIP_TRY(ctx, hipMemsetAsync(d_sched_ctl, 0, sizeof(int32_t) * 8, s0));
    for (StreamGroup& g : groups) {
        HIP_TRY(ctx, hipMemsetAsync(g.d_slot_win, 0xFF, sizeof(int32_t) * std::max(1, g.n_slots), s0));
        for (int i = 0; i < 4; ++i) g.h_done[i] = 0;
    }
    HIP_TRY(ctx, hipEventRecord(start_ev, s0));
    for (size_t gi = 1; gi < groups.size(); ++gi) HIP_TRY(ctx, hipStreamWaitEvent(groups[gi].stream, start_ev, 0));
    const bool time_kernels = groups.size() == 1;  // kernel timing by events is only meaningful without overlap
    constexpr int kLag = 2;
    // KBA_SCHED_TRACE=1 (profiling aid): windows finished as of every round -> how full the slots are over the solve
    static const bool sched_trace = std::getenv("KBA_SCHED_TRACE") != nullptr;
    std::vector<int> done_curve;
    double enq_us = 0.0;  // host time inside enqueue_round (KBA_SCHED_TRACE)
    const auto t_solve0 = std::chrono::steady_clock::now();
    bool finished = false;
    int done_seen = 0;  // windows finished, as last read from the pinned ring (monotone, kLag + 1 rounds old when it is used)
    for (int round = 0; !finished; ++round) {
        const int in_flight_max = (int)P.n_win - done_seen;
        const auto t_enq0 = std::chrono::steady_clock::now();
        for (StreamGroup& g : groups) enqueue_round(g, round, time_kernels, in_flight_max);
        ++b.run.n_rounds;
        if (sched_trace) enq_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enq0).count();
        if (b.rc != LIMO_OK) break;
        if (round >= kLag) {
            finished = true;
            for (StreamGroup& g : groups) {
                b.note(hipEventSynchronize(g.round_ev[(round - kLag) & 3]), "sync round");
                if (b.rc != LIMO_OK) break;
                const int d = g.h_done[(round - kLag) & 3];
                if (d < P.n_win) finished = false;
                done_seen = std::max(done_seen, d);
            }
            if (sched_trace) done_curve.push_back(groups[0].h_done[(round - kLag) & 3]);
        }
        if (round > 200000) {
            b.rc = LIMO_ERR_RUNTIME;
            ctx->err = "streaming solve did not terminate";
            break;
        }
    }
    if (sched_trace && !done_curve.empty()) {
        // in flight at round r = min(n_slots, windows not finished); printed as deciles of the round count
        const int R = (int)done_curve.size();
        long long occ = 0;
        std::fprintf(stderr, "[kba] streaming solve: %d windows, %d slots, %d groups, %d rounds; in flight at 0,10,..100 %% of the rounds:", (int)P.n_win, n_slots, (int)groups.size(), R);
        for (int r = 0; r < R; ++r) occ += std::min(n_slots, (int)P.n_win - done_curve[r]);
        for (int d = 0; d <= 10; ++d) std::fprintf(stderr, " %d", std::min(n_slots, (int)P.n_win - done_curve[std::min(R - 1, d * R / 10)]));
        std::fprintf(stderr, "; mean occupancy %.3f; host: %.1f us per round inside the enqueue calls, %.1f us per round wall\n", (double)occ / ((double)R * n_slots),
                     enq_us / (R + kLag), std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_solve0).count() / (R + kLag));
    }
    for (StreamGroup& g : groups) {  // everything joins the context's stream again
        b.note(hipStreamWaitEvent(g.stream, g.trim_ev, 0), "wait trim");
        if (g.stream != s0) {
            b.note(hipEventRecord(g.done_ev, g.stream), "record done");
            b.note(hipStreamWaitEvent(s0, g.done_ev, 0), "wait group");
        }
    }
    return b.rc;
}
