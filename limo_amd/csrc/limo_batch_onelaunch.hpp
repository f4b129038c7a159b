// limo_batch_onelaunch.hpp — the solves of a batch that are ONE launch (OneLaunch): k_solve_wg, k_solve_coop, and what follows a
// cooperative launch whose device-wide barrier was not met in time.  Part of limo_batch.hpp.
#pragma once

inline long long OneLaunch::cap_ticks() const {
    return b.opts.max_solver_time_sec > 0.0 ? std::max(1ll, (long long)(b.opts.max_solver_time_sec * 1e8)) : 0ll;
}
inline void OneLaunch::solve_wg() {
    const int lds = b.plan.onelaunch_lds;
    b.note(hipFuncSetAttribute((const void*)k_solve_wg, hipFuncAttributeMaxDynamicSharedMemorySize, lds), "hipFuncSetAttribute(k_solve_wg)");
    hipLaunchKernelGGL(k_solve_wg, dim3(b.P.n_win), dim3(kBlock), lds, b.ctx->stream, b.bv, b.c, cap_ticks(), b.d_plane_rep, b.d_plane_dep);
    b.launch_check("k_solve_wg");
}

// false: the launch was refused (nothing ran) - the caller takes the launch sequence
inline bool OneLaunch::solve_coop(const CoopGeometry& geo) {
    limo_ctx* ctx = b.ctx;
    const PackedBatch& P = b.P;
    const BatchPlan& plan = b.plan;
    const int lds = coop_lds_bytes(plan);
    if (!d_coop_bar && b.dmalloc((void**)&d_coop_bar, sizeof(int32_t) * 8 * P.n_win)) return false;
    if (!d_coop_red && b.dmalloc((void**)&d_coop_red, sizeof(double) * kCoopRedStride * P.n_win)) return false;
    if (hipFuncSetAttribute((const void*)k_solve_coop, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    b.note(hipMemsetAsync(d_coop_bar, 0, sizeof(int32_t) * 8 * P.n_win, ctx->stream), "memset barrier words");
    if (b.spart_has_packed) {
        b.note(hipMemsetAsync(b.bv.S_part, 0, sizeof(double) * (size_t)std::max<int64_t>(1, P.spart_total), ctx->stream), "clear packed Schur slabs");
        b.spart_has_packed = false;
    }
    b.h_pin->coop_abort = 0;
    CoopParams cp;
    cp.G = geo.G;
    cp.vp = plan.plain_tm;
    cp.vg = plan.gp_tm;
    cp.schur_lds = plan.schur_wave_lds / (int)sizeof(double);
    cp.cap_ticks = cap_ticks();
    // barrier timeout in ticks of the 100 MHz constant clock (KBA_COOP_TIMEOUT_MS=0: give up at the first wait - how the tests
    // reach recover())
    // default 50 ms (the whole call is ~5 ms; the longest phase between two barriers - the quantile trimming - well under 1 ms):
    // a barrier that is not met by then is lost, and the caller of a 10 Hz pipeline should not wait seconds to learn it
    cp.timeout_ticks = std::max(0ll, (long long)(b.run.sw.coop_timeout_ms * 1e5));
    cp.bar = d_coop_bar;
    cp.abort_host = &b.d_pin->coop_abort;
    cp.plane_rep = b.d_plane_rep;
    cp.plane_dep = b.d_plane_dep;
    cp.red = d_coop_red;
    SolveConsts cc = b.c;
    cc.slab_packed = 0;  // (tile layout: the slab sum of k_solve_coop indexes it)
    void* args[] = {(void*)&b.bv, (void*)&cc, (void*)&cp};
    // A PLAIN launch, with the co-residency of the grid checked here against the occupancy the runtime reports (the workgroups
    // of other kernels on the device all finish, so every workgroup of this grid gets its CU; a barrier that waits too long is
    // recovered, coop_sync).  hipLaunchCooperativeKernel gives the same guarantee from the runtime, but after the first such launch
    // of a process every LATER solve that uses several streams ran 30-50 % slower (a 2048-window batch 91 -> 118-137 ms,
    // profiles/r04_experiment_coop_api_vs_plain_launch.txt).
    int per_cu = 0, n_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_solve_coop, kBlock, (size_t)lds) != hipSuccess ||
        hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || per_cu * n_cu < geo.grid) {
        (void)hipGetLastError();
        return false;  // (not all workgroups resident at once: the launch sequence)
    }
    if (hipLaunchKernel((const void*)k_solve_coop, dim3(geo.grid), dim3(kBlock), args, lds, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    coop_launched = true;
    return true;
}

// Behind the path of a solve.  A device-wide barrier of k_solve_coop that was not met in time aborts the launch
// (kba_kernels.hip:coop_sync) and leaves poses, landmarks and LM state half-updated.  That is recoverable: the batch's initial state
// is restored (the pristine copies limo_ba_batch_reset uses) and the same windows go through the launch sequence - same results,
// bit for bit.  Returns 1: the state is restored, the caller runs the launch sequence; 0: nothing to do; < 0: a limo_status.
inline int OneLaunch::recover() {
    if (!coop_launched) return 0;
    limo_ctx* ctx = b.ctx;
    coop_launched = false;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (b.h_pin->coop_abort == 0) {
        ctx->coop_strikes = 0;
        return 0;
    }
    b.h_pin->coop_abort = 0;
    b.run.coop_redone = true;
    ++ctx->coop_fallbacks;
    ++ctx->coop_strikes;
    if (b.reset_state() != LIMO_OK) return LIMO_ERR_RUNTIME;
    b.rc = LIMO_OK;
    return 1;
}
