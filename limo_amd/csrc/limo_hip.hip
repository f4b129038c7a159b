// limo_hip.hip — the C-ABI of include/limo_hip.h on top of the gfx950 kernels (kba_kernels.hip).
// Host side: packing (kba_pack.cpp), device allocation, launch sequencing, result download.
// There is NO CPU fallback here: without a HIP device limo_ctx_create fails with LIMO_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "kba_kernels.hip"

#include "kba_batch_plan.hpp"
#include "kba_buffers.hpp"
#include "kba_rows.hpp"

using namespace kba;

#include "limo_ctx.hpp"

#define HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                     \
            return LIMO_ERR_RUNTIME;                                                             \
        }                                                                                        \
    } while (0)

namespace {

inline int cdiv(int64_t a, int64_t b) {
    return (int)((a + b - 1) / b);
}

struct EventPair {
    hipEvent_t a, b;
    int kernel;  // LIMO_KERNEL_*
};

}  // namespace

struct limo_ba_batch : Executor {
    limo_ctx* ctx = nullptr;
    PackedBatch P;
    bool holds_pack_arena = false;  // P's big arrays live in ctx->pack_arena
    bool pose_batch = false;        // made by limo_ba_batch_create_pose_only: limo_ba_batch_solve picks its launch path by that
    BatchView bv;
    SolveConsts c;
    limo_ba_options opts;
    std::vector<std::pair<void*, size_t>> allocs;  // device blocks of this batch (returned to the context's pool)
    double *d_plane_rep = nullptr, *d_plane_dep = nullptr;
    double *d_pose0 = nullptr, *d_pdir0 = nullptr, *d_pdist0 = nullptr, *d_lm0 = nullptr;
    uint8_t* d_lm_state0 = nullptr;
    std::vector<WinState> st0;  // reset image of the LM state
    int32_t* h_active = nullptr;  // pinned, 4 slots: written by k_cam_assemble, read by the host one iteration later
    int32_t* d_h_active = nullptr;  // the same words as the device sees them
    size_t h_flags_bytes = 0;
    hipEvent_t act_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int it_no = 0;
    // The workgroups a producer view pv[i] launches (a null list = every workgroup, in order).  `full` lists every window - of an
    // unsharded batch without any list but the Schur one, which is built on first use (the one-launch and streaming solves never
    // need it); of a shard, the workgroups it owns.  `cur` is what the lock-step launches use: `full`, or the lists of the windows
    // that still iterate - rebuilt on the host whenever the active set has halved, so late LM iterations only launch the workgroups
    // that have work (rebatch).
    // Schur worklists are ordered [plain groups of fast windows | ground-plane groups of fast windows | generic windows]
    struct WorkLists {
        const int32_t *blk = nullptr, *lblk = nullptr, *sblk = nullptr, *win = nullptr;
        int n_blk = 0, n_lblk = 0, n_sblk_plain = 0, n_sblk_fgp = 0, n_sblk = 0, n_win = 0;
    };
    struct ViewLists {
        WorkLists full, cur;
        int owner = -1;  // shard whose Schur blocks the view lists (-1: all of them)
    };
    std::vector<ViewLists> wl;  // [pv.size()]
    int32_t *d_act_blk = nullptr, *d_act_lblk = nullptr, *d_act_sblk = nullptr, *d_act_win = nullptr;  // device lists of a re-batched active set
    int32_t* d_flags = nullptr;
    BatchPlan plan;  // kernel variants and LDS sizes (kba_batch_plan.hpp) ...
    const void *schur_fn_plain = nullptr, *schur_fn_leangp = nullptr, *schur_fn_gen = nullptr;  // ... and the variants as kernels
    const void* schur_fn_narrow = nullptr;  // plan.narrow: k_schur_lean_gp
    bool gp_wide = false;                   // SolveSwitches::gp_wide of the solve in progress
    bool schur_pair_ok = false;      // plan.pair_ok, and KBA_NO_SCHUR_PAIR is not set
    static constexpr int kSchurPairBound = 384;  // windows in flight in a slot group up to which a round launches the pair kernel (192: -0.7 %, 768: -9 % at 1024 windows)
    int32_t* h_flags = nullptr;  // pinned
    int rc = LIMO_OK;
    // ---- streaming solve (device-side scheduler k_sched): windows move through n_slots slots, a finished window is
    // replaced by the next pending one, so every launch round works on a full set (kba_kernels.hip:k_sched)
    int n_slots = 0;
    int32_t* d_sched_ctl = nullptr;   // [0] cursor over the batch's windows, [1] windows finished (shared by the groups)
    // ---- landmark sharding.  shard_P == 1: everything below is inert (pv = {bv}, local_shards = {0}).
    // Every shard holds the same global layout and owns the observation / landmark / Schur workgroups of its
    // landmarks (rank lists); the per-workgroup partial arrays it produces live in its own "producer view" pv[i] and
    // are summed into the consumer view bv before each window-level kernel: by RCCL all-reduce when the shards are
    // ranks (one local shard), by k_sum_shards when all shards are virtual on this GPU.
    int shard_P = 1, shard_rank = 0;
    bool shard_virtual = true;
    std::vector<int> local_shards;
    std::vector<BatchView> pv;
    ExchangeLayout xl;
    double* arena_c = nullptr;          // consumer view: the P contributions side by side (kba_buffers.hpp:exchange_layout)
    std::vector<double*> blocks;        // block of local shard i (what it contributes per LM iteration)
    std::vector<double*> trims;         // trimming arenas: [0] consumer, [1 + i] local shard i
    double* d_gather = nullptr;         // [world][block] staging of the all-gather
    WinDesc* d_win_orig = nullptr;      // the batch's own window descriptors (bv.win of the consumer view is modified)
    bool first_lin = false, assemble_pending = false;
    int64_t n_exchanges = 0, exchange_bytes = 0;  // all-reduce calls / bytes of this batch so far (limo_ba_batch_exchange_stats)
    double* d_lm_tmp = nullptr;
    // kernel timing (linearize) via HIP events on the batch's stream
    std::vector<EventPair> ev_pool;
    size_t ev_used = 0;
    double k_ms_acc[2] = {0.0, 0.0};      // indexed by LIMO_KERNEL_LINEARIZE / LIMO_KERNEL_SCHUR
    int64_t k_launches[2] = {0, 0};
    hipEvent_t ev_total_a = nullptr, ev_total_b = nullptr;
    double total_ms_acc = 0.0;
    double last_solve_sec = 0.0;
    // what limo_ctx_last_solve_info tells about the solve in progress beyond its path (reset by limo_ba_batch_solve)
    int64_t n_rounds = 0, n_pair_launches = 0;
    int64_t n_narrow_launches = 0, n_widegp_launches = 0;  // launches that ran narrow / three-panel ground-plane waves (limo_ctx_last_schur_gp_info)
    int lin_variant = 1;  // k_lin_lm<true> / <false> of the last launch; the one-launch kernels always linearise through LDS
    // lanes of the camera kernels (kba_batch_plan.hpp:plan_cam_lanes / cam_lanes_for_launch; limo_ctx_last_cam_lanes_info)
    CamOccupancy cam_occ;
    CamLanesPlan cam_plan;
    int cam_lanes_forced = 0;              // SolveSwitches::cam_lanes of the solve in progress
    int64_t n_cam_launches[2][2] = {{0, 0}, {0, 0}};  // [assemble, solve][half, full] launches of the solve in progress

    ~limo_ba_batch() override {
        // (the arrays of P that live in the context's pinned pack arena are not freed one by one - kba_pack.hpp:PackArena -, the arena
        // is free for the next batch from here on; whatever of this batch's upload is still in flight only feeds device blocks that
        // go back to the pool below and are rewritten, in stream order, by their next user)
        if (holds_pack_arena) ctx->pack_arena_busy = false;
        for (auto& a : allocs) ctx->pool_free(a.first, a.second);
        if (h_active) ctx->host_free(h_active, 64);
        if (h_flags) ctx->host_free(h_flags, h_flags_bytes);
        stream_teardown();
        for (auto& e : ev_pool) {
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
        for (auto& e : act_ev)
            if (e) (void)hipEventDestroy(e);
        if (ev_total_a) (void)hipEventDestroy(ev_total_a);
        if (ev_total_b) (void)hipEventDestroy(ev_total_b);
    }

    int dmalloc(void** p, size_t bytes) {
        bytes = bytes ? bytes : 8;
        HIP_TRY(ctx, ctx->pool_alloc(p, bytes));
        allocs.push_back({*p, bytes});
        // debugging aid: KBA_POISON=1 fills every block with NaN bytes first, so that a kernel reading a word nobody
        // wrote shows up as a wrong result instead of depending on what the block held before
        static const bool poison = std::getenv("KBA_POISON") != nullptr;
        if (poison) {
            HIP_TRY(ctx, hipMemsetAsync(*p, 0xFF, bytes, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return LIMO_OK;
    }

    // The kernel of a plan entry: cls 0 / 1 = k_schur_lean<a, false / true, b> (a = TM, b = waves per EU), cls 2 = k_schur_wide<a>.
    static const void* schur_kernel(int cls, int a, int b) {
        switch (cls * 100 + a * 10 + b) {
            case 14: return (const void*)k_schur_lean<1, false, 4>;
            case 23: return (const void*)k_schur_lean<2, false, 3>;
            case 113: return (const void*)k_schur_lean<1, true, 3>;
            case 122: return (const void*)k_schur_lean<2, true, 2>;
            case 132: return (const void*)k_schur_lean<3, true, 2>;
            case 210: return (const void*)k_schur_wide<1>;
            case 230: return (const void*)k_schur_wide<3>;
            case 260: return (const void*)k_schur_wide<6>;
            case 320: return (const void*)k_schur_wide<12>;
        }
        return nullptr;
    }

    // A worklist as a device block of this batch (a synchronous copy).
    int upload_list(const std::vector<int32_t>& v, const int32_t** out) {
        int32_t* d = nullptr;
        if (dmalloc((void**)&d, sizeof(int32_t) * std::max<size_t>(1, v.size()))) return LIMO_ERR_RUNTIME;
        if (!v.empty()) HIP_TRY(ctx, hipMemcpy(d, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice));
        *out = d;
        return LIMO_OK;
    }
    // The Schur worklist of every window, for producer view i.
    int build_full_sblk(size_t i) {
        WorkLists& f = wl[i].full;
        std::vector<int32_t> v;
        build_sblk_list(P, nullptr, c.schur_span, c.schur_span_gp, wl[i].owner, v, f.n_sblk_plain, f.n_sblk_fgp);
        f.n_sblk = (int)v.size();
        return upload_list(v, &f.sblk);
    }

    int upload() {
        std::memset(&bv, 0, sizeof(bv));
        // Every buffer of the batch view lives in ONE device block: [initialised buffers | zero-filled buffers].
        // Small batches (a single window) stage the initialised part in pinned host memory and upload it with one
        // copy; large ones copy buffer by buffer (no second host copy of hundreds of MB).  One memset for the rest.
        int status = LIMO_OK;
        struct Ent {
            void** slot;
            size_t bytes, off;
            const void* init;
        };
        std::vector<Ent> ents;
        for_each_buffer(P, bv, [&](void** slot, size_t bytes, const void* init) { ents.push_back({slot, bytes ? bytes : 8, 0, init}); });
        // the LM state starts from its reset image (reset_state restores exactly this), uploaded with everything else: a
        // fresh batch needs no reset pass (six copies and a stream drain per single-window call)
        st0.assign(P.n_win, WinState());
        std::memset(st0.data(), 0, sizeof(WinState) * st0.size());
        for (auto& q : st0) q.term = -1;
        for (Ent& e : ents)
            if (e.slot == (void**)&bv.st) e.init = st0.data();
        // the pristine copies limo_ba_batch_reset restores from
        ents.push_back({(void**)&d_pose0, sizeof(double) * 7 * std::max(1, P.TK), 0, P.pose.empty() ? nullptr : P.pose.data()});
        ents.push_back({(void**)&d_pdir0, sizeof(double) * 3 * std::max(1, P.TK), 0, P.pdir.empty() ? nullptr : P.pdir.data()});
        ents.push_back({(void**)&d_pdist0, sizeof(double) * std::max(1, P.TK), 0, P.pdist.empty() ? nullptr : P.pdist.data()});
        ents.push_back({(void**)&d_lm0, sizeof(double) * 3 * std::max(1, P.TL), 0, P.lm.empty() ? nullptr : P.lm.data()});
        ents.push_back({(void**)&d_lm_state0, (size_t)std::max(1, P.TL), 0, P.lm_state.empty() ? nullptr : P.lm_state.data()});
        auto align = [](size_t x) { return (x + 255) / 256 * 256; };
        size_t init_total = 0, zero_total = 0;
        for (Ent& e : ents)
            if (e.init) {
                e.off = init_total;
                init_total += align(e.bytes);
            }
        for (Ent& e : ents)
            if (!e.init) {
                e.off = init_total + zero_total;
                zero_total += align(e.bytes);
            }
        char* arena = nullptr;
        if (dmalloc((void**)&arena, init_total + zero_total)) return LIMO_ERR_RUNTIME;
        for (Ent& e : ents) *e.slot = arena + e.off;
        constexpr size_t kStageMax = 16u << 20;
        if (init_total <= kStageMax) {
            HIP_TRY(ctx, ctx->staging.ensure(init_total, 1u << 20));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // an earlier upload may still read the staging buffer
            for (const Ent& e : ents)
                if (e.init) std::memcpy(static_cast<char*>(ctx->staging.p) + e.off, e.init, e.bytes);
            if (init_total) HIP_TRY(ctx, hipMemcpyAsync(arena, ctx->staging.p, init_total, hipMemcpyHostToDevice, ctx->stream));
        } else {
            // (a host array that initialises several device buffers - the landmarks: current, candidate and pristine copy - crosses the
            // bus ONCE and is copied on the device for the others: 96 MB of 390 less for 1024 C2 windows, 12.2 -> ~9 ms)
            for (size_t i = 0; i < ents.size(); ++i) {
                const Ent& e = ents[i];
                if (!e.init) continue;
                const Ent* first = nullptr;
                for (size_t j = 0; j < i && !first; ++j)
                    if (ents[j].init == e.init && ents[j].bytes == e.bytes) first = &ents[j];
                if (first)
                    HIP_TRY(ctx, hipMemcpyAsync(arena + e.off, arena + first->off, e.bytes, hipMemcpyDeviceToDevice, ctx->stream));
                else
                    HIP_TRY(ctx, hipMemcpyAsync(arena + e.off, e.init, e.bytes, hipMemcpyHostToDevice, ctx->stream));
            }
        }
        if (zero_total) HIP_TRY(ctx, hipMemsetAsync(arena + init_total, 0, zero_total, ctx->stream));
        if (status != LIMO_OK) return status;
        // the measurements at the pair's index, from the slot table and the observations that have just been uploaded (the same stream)
        if (!P.evaluate_only && P.pair_m.empty()) {
            const int64_t n_pair = (int64_t)P.lm_slot.size();
            hipLaunchKernelGGL(k_pair_fill, dim3((unsigned)((n_pair + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, bv, n_pair);
            HIP_TRY(ctx, hipGetLastError());
        }
        pv.assign(1, bv);
        if (shard_P > 1) {
            xl = exchange_layout(P);
            d_win_orig = const_cast<WinDesc*>(bv.win);
            pv.assign(local_shards.size(), bv);  // producers keep the batch's own per-workgroup arrays (every entry has ONE owner)
            auto zeros = [&](double** out, size_t n) -> int {
                if (dmalloc((void**)out, sizeof(double) * std::max<size_t>(1, n))) return LIMO_ERR_RUNTIME;
                HIP_TRY(ctx, hipMemsetAsync(*out, 0, sizeof(double) * std::max<size_t>(1, n), ctx->stream));
                return LIMO_OK;
            };
            if (zeros(&arena_c, xl.c_total)) return LIMO_ERR_RUNTIME;
            trims.assign(1 + local_shards.size(), nullptr);
            for (double*& t : trims)
                if (zeros(&t, xl.trim_count)) return LIMO_ERR_RUNTIME;
            blocks.assign(local_shards.size(), nullptr);
            if (!shard_virtual && zeros(&d_gather, (size_t)ctx->comm_world * xl.b_total)) return LIMO_ERR_RUNTIME;
            {   // consumer view: "P workgroups, P rows" per window
                std::vector<WinDesc> wc = exchange_consumer_windows(P);
                WinDesc* d_wc = nullptr;
                if (dmalloc((void**)&d_wc, sizeof(WinDesc) * wc.size())) return LIMO_ERR_RUNTIME;
                HIP_TRY(ctx, hipMemcpy(d_wc, wc.data(), sizeof(WinDesc) * wc.size(), hipMemcpyHostToDevice));
                exchange_bind_consumer(xl, bv, arena_c, trims[0], d_wc);
            }
            for (size_t i = 0; i < local_shards.size(); ++i) {
                if (zeros(&blocks[i], xl.b_total)) return LIMO_ERR_RUNTIME;  // the shard's own block ...
                exchange_bind_producer(xl, pv[i], blocks[i], trims[1 + i]);
                if (zeros(&pv[i].S_part, xl.spart_count)) return LIMO_ERR_RUNTIME;  // ... and its private Schur slabs
            }
            if (!shard_virtual && dmalloc((void**)&d_lm_tmp, sizeof(double) * 3 * std::max(1, P.TL))) return LIMO_ERR_RUNTIME;
        }
        if (dmalloc((void**)&d_plane_rep, sizeof(double) * P.SO)) return LIMO_ERR_RUNTIME;
        if (dmalloc((void**)&d_plane_dep, sizeof(double) * P.SO)) return LIMO_ERR_RUNTIME;
        HIP_TRY(ctx, ctx->host_alloc((void**)&h_active, 64));
        HIP_TRY(ctx, hipHostGetDevicePointer((void**)&d_h_active, h_active, 0));
        bv.n_active_host = nullptr;
        h_flags_bytes = sizeof(int32_t) * std::max(1, P.n_win);
        HIP_TRY(ctx, ctx->host_alloc((void**)&h_flags, h_flags_bytes));
        if (dmalloc((void**)&d_act_blk, sizeof(int32_t) * std::max(1, P.n_blk))) return LIMO_ERR_RUNTIME;
        if (dmalloc((void**)&d_act_lblk, sizeof(int32_t) * std::max(1, P.n_lblk))) return LIMO_ERR_RUNTIME;
        if (dmalloc((void**)&d_act_sblk, sizeof(int32_t) * std::max(1, P.n_sblk))) return LIMO_ERR_RUNTIME;
        if (dmalloc((void**)&d_act_win, sizeof(int32_t) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
        if (dmalloc((void**)&d_flags, sizeof(int32_t) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
        // full lists: a shard's are its own workgroups (Schur blocks: span 1), built here; an unsharded batch needs none but the
        // Schur list, which waits for its first lock-step solve (full_lists)
        wl.assign(pv.size(), ViewLists());
        for (size_t i = 0; i < wl.size(); ++i) {
            WorkLists& f = wl[i].full;
            f.n_blk = P.n_blk;
            f.n_lblk = P.n_lblk;
            f.n_win = P.n_win;
            if (shard_P == 1) continue;
            const int r = wl[i].owner = local_shards[i];
            auto owned = [&](const std::vector<int32_t>& owner, const int32_t** list, int* n) -> int {
                std::vector<int32_t> v;
                for (size_t k = 0; k < owner.size(); ++k)
                    if (owner[k] == r) v.push_back((int32_t)k);
                *n = (int)v.size();
                return upload_list(v, list);
            };
            if (owned(P.blk_owner, &f.blk, &f.n_blk) || owned(P.lblk_owner, &f.lblk, &f.n_lblk) || build_full_sblk(i)) return LIMO_ERR_RUNTIME;
        }
        plan = plan_batch(P, {schur_lean_lds_bytes, schur_wide_lds_bytes, lin_lm_lds_bytes(P.Vmax, true), kWideWaves, kTrimMaxSort});
        if (plan.wide_npw < 0) {
            ctx->err = "window with too many free camera slots for k_schur_wide";
            return LIMO_ERR_INVALID;
        }
        if (plan.any_fast) {
            schur_fn_plain = schur_kernel(0, plan.plain_tm, plan.plain_wpe);
            HIP_TRY(ctx, hipFuncSetAttribute(schur_fn_plain, hipFuncAttributeMaxDynamicSharedMemorySize, plan.plain_lds));
            schur_fn_leangp = schur_kernel(1, plan.gp_tm, plan.gp_wpe);
            HIP_TRY(ctx, hipFuncSetAttribute(schur_fn_leangp, hipFuncAttributeMaxDynamicSharedMemorySize, plan.leangp_lds));
            schur_pair_ok = plan.pair_ok && !(std::getenv("KBA_NO_SCHUR_PAIR") && std::atoi(std::getenv("KBA_NO_SCHUR_PAIR")) != 0);
            if (schur_pair_ok)
                HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_schur_lean_pair<2, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, std::max(plan.plain_lds, plan.leangp_lds)));
            if (plan.narrow) {
                schur_fn_narrow = (const void*)k_schur_lean_gp;
                HIP_TRY(ctx, hipFuncSetAttribute(schur_fn_narrow, hipFuncAttributeMaxDynamicSharedMemorySize, plan.leangp_lds));
                if (schur_pair_ok)
                    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_schur_lean_pair<2, 3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, std::max(plan.plain_lds, plan.leangp_lds)));
            }
        }
        if (plan.any_gen) {
            schur_fn_gen = schur_kernel(2, plan.wide_npw, 0);
            HIP_TRY(ctx, hipFuncSetAttribute(schur_fn_gen, hipFuncAttributeMaxDynamicSharedMemorySize, plan.wide_lds));
        }
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_cam_assemble<kBlock>, hipFuncAttributeMaxDynamicSharedMemorySize, plan.asm_bytes));
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_cam_solve<kBlock>, hipFuncAttributeMaxDynamicSharedMemorySize, plan.solve_bytes));
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_cam_assemble<kCamLanesHalf>, hipFuncAttributeMaxDynamicSharedMemorySize, plan.asm_bytes));
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_cam_solve<kCamLanesHalf>, hipFuncAttributeMaxDynamicSharedMemorySize, plan.solve_bytes));
        {   // which form of the two the batch may take (kba_batch_plan.hpp:plan_cam_lanes): workgroups per CU of the four instances
            HIP_TRY(ctx, hipDeviceGetAttribute(&cam_occ.n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
            HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&cam_occ.asm_full, k_cam_assemble<kBlock>, kBlock, plan.asm_bytes));
            HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&cam_occ.asm_half, k_cam_assemble<kCamLanesHalf>, kCamLanesHalf, plan.asm_bytes));
            HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&cam_occ.solve_full, k_cam_solve<kBlock>, kBlock, plan.solve_bytes));
            HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&cam_occ.solve_half, k_cam_solve<kCamLanesHalf>, kCamLanesHalf, plan.solve_bytes));
            cam_plan = plan_cam_lanes(P, cam_occ, shard_P == 1 && !pose_batch);
        }
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_trim_select, hipFuncAttributeMaxDynamicSharedMemorySize, plan.trim_bytes));
        for (auto& e : act_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreate(&ev_total_a));
        HIP_TRY(ctx, hipEventCreate(&ev_total_b));
        return LIMO_OK;
    }

    // S_part holds packed slabs (SolveConsts::slab_packed) of an earlier solve of this batch.  The tile layout counts on the zeros of
    // the allocation in the tiles a plain group never writes (the slab sums read them for the up to three plain slabs behind q_gp),
    // and packed slabs lie across such tiles: the one-launch solve clears the buffer first (a solve after limo_ba_batch_reset that
    // follows a warm re-solve - rare, and a fill of a few MB)
    bool spart_has_packed = false;
    bool pristine = true;  // the device state is the state of create / reset: what a recovered barrier timeout of the one-launch solve restores
    int reset_state() {
        pristine = true;
        HIP_TRY(ctx, hipMemcpyAsync(bv.st, st0.data(), sizeof(WinState) * st0.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(bv.pose, d_pose0, sizeof(double) * 7 * P.TK, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(bv.pdir, d_pdir0, sizeof(double) * 3 * P.TK, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(bv.pdist, d_pdist0, sizeof(double) * P.TK, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(bv.lm, d_lm0, sizeof(double) * 3 * P.TL, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(bv.lm_state, d_lm_state0, P.TL, hipMemcpyDeviceToDevice, ctx->stream));
        return LIMO_OK;
    }

    // ---- iteration log (limo_hip.h:limo_ba_iteration; kba_lm.hpp:lm_log_push).  limo_ba_batch_solve binds it when the context's
    // switch is on: every window gets the exact bound of the schedule as its capacity, the reset image carries the pointers (so
    // limo_ba_batch_reset and a recovered barrier timeout start the log again at zero entries), k_log_bind puts them into the live state.
    limo_ba_iteration* d_log = nullptr;
    int log_cap = 0;    // entries per window of the binding in force; 0: no log
    int log_alloc = 0;  // entries per window d_log has room for
    static int log_bound(const limo_ba_options& o) {
        const int64_t t = std::max(0, o.trim_solver_iterations), r = std::max(0, o.num_trim_rounds), m = std::max(0, o.max_num_iterations);
        return (int)std::min<int64_t>(r * ((t + 1) + (3 * t + 1)) + (m + 1), 1 << 24);
    }
    int bind_log(bool on) {
        const int cap = on ? log_bound(opts) : 0;
        if (!on && !log_cap) return LIMO_OK;  // (never bound, or unbound already: the state holds no pointer)
        if (cap > log_alloc) {
            if (dmalloc((void**)&d_log, sizeof(limo_ba_iteration) * (size_t)cap * (size_t)std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
            log_alloc = cap;
        }
        if (cap != log_cap) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier reset may still read the image)
            for (int w = 0; w < P.n_win; ++w) {
                st0[w].log = on ? d_log + (size_t)w * cap : nullptr;
                st0[w].log_cap = cap;
            }
            log_cap = cap;
        }
        hipLaunchKernelGGL(k_log_bind, dim3(cdiv(P.n_win, 256)), dim3(256), 0, ctx->stream, bv, on ? d_log : (limo_ba_iteration*)nullptr, cap);
        HIP_TRY(ctx, hipGetLastError());
        return LIMO_OK;
    }
    // entries of window w -> host: *n = what the window has, at most `cap` written
    int read_log(int w, int cap, limo_ba_iteration* out, int32_t* n) {
        *n = 0;
        if (!log_cap) return LIMO_OK;
        WinState s;
        HIP_TRY(ctx, hipMemcpyAsync(&s, bv.st + w, sizeof(WinState), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const int have = std::max(0, std::min(s.log_n, log_cap)), m = std::min(have, cap);
        *n = have;
        if (m > 0) {
            HIP_TRY(ctx, hipMemcpyAsync(out, d_log + (size_t)w * log_cap, sizeof(limo_ba_iteration) * m, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return LIMO_OK;
    }
    // every window's entries into the context's buffer (limo_ctx_last_iteration_log), for the calls that destroy their batch
    int export_log() {
        ctx->last_log.clear();
        ctx->last_log_n.clear();
        ctx->last_log_off.clear();
        if (!log_cap) return LIMO_OK;
        std::vector<WinState> sv(P.n_win);
        HIP_TRY(ctx, hipMemcpyAsync(sv.data(), bv.st, sizeof(WinState) * sv.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        size_t total = 0;
        for (int w = 0; w < P.n_win; ++w) {
            const int have = std::max(0, std::min(sv[w].log_n, log_cap));
            ctx->last_log_n.push_back(have);
            ctx->last_log_off.push_back(total);
            total += (size_t)have;
        }
        ctx->last_log.resize(total);
        for (int w = 0; w < P.n_win; ++w)
            if (ctx->last_log_n[w])
                HIP_TRY(ctx, hipMemcpyAsync(ctx->last_log.data() + ctx->last_log_off[w], d_log + (size_t)w * log_cap,
                                            sizeof(limo_ba_iteration) * ctx->last_log_n[w], hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return LIMO_OK;
    }

    void note(hipError_t e, const char* what) {
        if (e != hipSuccess && rc == LIMO_OK) {
            rc = LIMO_ERR_RUNTIME;
            ctx->err = std::string(what) + ": " + hipGetErrorString(e);
        }
    }
    void note_nccl(ncclResult_t r, const char* what) {
        if (r != ncclSuccess && rc == LIMO_OK) {
            rc = LIMO_ERR_RUNTIME;
            ctx->err = std::string(what) + ": " + ncclGetErrorString(r);
        }
    }
#define LAUNCH_CHECK(what) note(hipGetLastError(), what)

    // ---- Executor
    // The constants of a solve with options `o`: make_consts plus what depends on the batch's sharding alone (fixed at creation).
    // Schur granularity: a wave takes two plain Schur blocks (128 landmarks, 8 tiles) or one ground-plane block.  Fixed
    // (not a function of how many windows are in flight): the partial-slab layout of a window, and with it the order in
    // which its Schur complement is summed, is then the same alone and inside any batch - single-window and batched
    // solves give the same bits.  (Measured at 1024 C2 windows: span 2 is as fast as 4, span 1 costs 2 %.)
    // The spans also decide which slabs of S_part are "plain" (written in part only, kba_kernels.hip:schur_lean_group) - a slab must keep
    // its class for the life of the batch.
    SolveConsts consts_for(const limo_ba_options& o) const {
        SolveConsts k = make_consts(o);
        const bool sharded = shard_P > 1;
        k.schur_span = sharded ? 1 : kSchurSpan;  // (Schur blocks are cut at shard boundaries)
        k.schur_span_gp = kSchurSpanGp;
        k.schur_nslab = sharded ? shard_P : 0;
        k.schur_packed = sharded ? 1 : 0;
        // the launch sequences of an unsharded batch (lock-step and streaming) keep the partial slabs of fast-class windows packed
        // (kba_items.hpp:slab_packed_write); a sharded solve reduces tile slabs (slab_reduce_entry), and the one-launch solve, whose
        // own slab sum indexes the tile layout, gets a copy of the constants without it (solve_coop)
        k.slab_packed = sharded ? 0 : 1;
        return k;
    }

    // Per-iteration exchange (point 1 = A1, 2 = A2, 3 = A, 4 = B; kba_buffers.hpp:exchange_layout): ALL-GATHER of the shards'
    // blocks over the ranks - one call per local slot, normally one shard per rank: ONE ncclAllGather of 41 KB at a C4 window -
    // then k_unpack puts every contribution at its shard's place in the consumer view.  Shard s lives on rank s mod world, in
    // local slot s / world.  Virtual shards (no communicator): the unpack alone.
    void exchange(int point) {
        if (shard_P == 1) return;
        hipStream_t s = ctx->stream;
        size_t off, count;
        xl.range(point, off, count);
        for (size_t i = 0; i < pv.size(); ++i) {
            if (shard_virtual) {
                hipLaunchKernelGGL(k_unpack, dim3(cdiv((int64_t)count, 256)), dim3(256), 0, s, xl, (const WinDesc*)d_win_orig, (const double*)(blocks[i] + off), arena_c,
                                   local_shards[i], (int64_t)off, (int64_t)count);
                LAUNCH_CHECK("k_unpack");
            } else {
                if (ctx->xfn) {
                    host_exchange(blocks[i] + off, d_gather, count, 0);
                } else {
                    note_nccl(ncclAllGather(blocks[i] + off, d_gather, count, ncclDouble, (ncclComm_t)ctx->comm, s), "ncclAllGather");
                }
                for (int q = 0; q < ctx->comm_world; ++q) {
                    hipLaunchKernelGGL(k_unpack, dim3(cdiv((int64_t)count, 256)), dim3(256), 0, s, xl, (const WinDesc*)d_win_orig,
                                       (const double*)(d_gather + (size_t)q * count), arena_c, (int)i * ctx->comm_world + q, (int64_t)off, (int64_t)count);
                    LAUNCH_CHECK("k_unpack");
                }
            }
            ++n_exchanges;
            exchange_bytes += (int64_t)count * (int64_t)sizeof(double);
        }
    }
    // The caller's transport (limo_ctx_comm_init_host): `count` doubles at `src` (device) go to the host, through the callback
    // (kind 0: all-gather into world * count doubles, rank order; kind 1: sum over the ranks into count doubles) and back to `dst`.
    void host_exchange(const double* src, double* dst, size_t count, int kind) {
        hipStream_t s = ctx->stream;
        const size_t n_out = kind == 0 ? (size_t)ctx->comm_world * count : count, need = count + n_out;
        if (ctx->xhost.ensure(sizeof(double) * need) != hipSuccess) {
            note(hipErrorOutOfMemory, "hipHostMalloc(exchange staging)");
            std::vector<double> z(need, 0.0);  // (the peers are still met: see below)
            ctx->xfn(z.data(), z.data() + count, (long long)count, kind, ctx->xuser);
            return;
        }
        double* const xhost = static_cast<double*>(ctx->xhost.p);
        // The transport is a COLLECTIVE: a rank that skipped it after a local error would leave its peers blocked in it for ever.  So
        // the call is made in every case - after an error with a zeroed contribution - and only the device copies are skipped; the
        // solve of this rank ends with LIMO_ERR_RUNTIME, the peers' solves end (with a result that misses this rank's share).
        if (rc == LIMO_OK) {
            note(hipMemcpyAsync(xhost, src, sizeof(double) * count, hipMemcpyDeviceToHost, s), "exchange: device -> host");
            note(hipStreamSynchronize(s), "exchange: sync");
        }
        if (rc != LIMO_OK) std::memset(xhost, 0, sizeof(double) * count);
        ctx->xfn(xhost, xhost + count, (long long)count, kind, ctx->xuser);
        if (rc != LIMO_OK) return;
        note(hipMemcpyAsync(dst, xhost + count, sizeof(double) * n_out, hipMemcpyHostToDevice, s), "exchange: host -> device");
        note(hipStreamSynchronize(s), "exchange: sync");  // (the staging buffer is reused by the next step)
    }
    // Trimming round: per-landmark residual maxima, one owner per entry and zero elsewhere - an exact sum in any order.
    void exchange_trim() {
        if (shard_P == 1) return;
        hipStream_t s = ctx->stream;
        const int64_t n = (int64_t)xl.trim_count;
        ShardPtrs sp;
        for (size_t i = 0; i < pv.size(); ++i) sp.p[i] = trims[1 + i];
        hipLaunchKernelGGL(k_sum_shards<double>, dim3(cdiv(n, 256)), dim3(256), 0, s, trims[0], sp, (int)pv.size(), n);
        LAUNCH_CHECK("k_sum_shards");
        if (!shard_virtual && ctx->xfn) {
            host_exchange(trims[0], trims[0], (size_t)n, 1);
        } else if (!shard_virtual) {
            note_nccl(ncclAllReduce(trims[0], trims[0], (size_t)n, ncclDouble, ncclSum, (ncclComm_t)ctx->comm, s), "ncclAllReduce");
        }
        ++n_exchanges;
        exchange_bytes += n * (int64_t)sizeof(double);
    }

    void full_lists() {
        for (size_t i = 0; i < wl.size(); ++i) {
            if (!wl[i].full.sblk && build_full_sblk(i) != LIMO_OK && rc == LIMO_OK) rc = LIMO_ERR_RUNTIME;
            wl[i].cur = wl[i].full;
        }
    }

    // Rebuild the worklists from the windows that are active right now (synchronises the stream).  Unsharded batches only: a sharded
    // batch has one window (batch_create_impl), and active_count() asks for eight.
    void rebatch() {
        if (shard_P > 1) return;
        hipStream_t s = ctx->stream;
        hipLaunchKernelGGL(k_export_active, dim3(cdiv(P.n_win, 256)), dim3(256), 0, s, bv, d_flags);
        note(hipMemcpyAsync(h_flags, d_flags, sizeof(int32_t) * P.n_win, hipMemcpyDeviceToHost, s), "memcpy flags");
        note(hipStreamSynchronize(s), "sync flags");
        if (rc != LIMO_OK) return;
        std::vector<int32_t> wb, wlb, wsb, ww;
        for (int w = 0; w < P.n_win; ++w) {
            if (!h_flags[w]) continue;
            const WinDesc& d = P.win[w];
            ww.push_back(w);
            for (int i = 0; i < d.n_blk; ++i) wb.push_back(d.blk0 + i);
            for (int i = 0; i < d.n_lblk; ++i) wlb.push_back(d.lblk0 + i);
        }
        WorkLists& a = wl[0].cur;
        build_sblk_list(P, &ww, c.schur_span, c.schur_span_gp, -1, wsb, a.n_sblk_plain, a.n_sblk_fgp);
        auto up = [&](int32_t* dst, const std::vector<int32_t>& v, const int32_t*& list, int& n) {
            if (!v.empty()) note(hipMemcpyAsync(dst, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice, s), "upload worklist");
            list = dst;
            n = (int)v.size();
        };
        up(d_act_blk, wb, a.blk, a.n_blk);
        up(d_act_lblk, wlb, a.lblk, a.n_lblk);
        up(d_act_sblk, wsb, a.sblk, a.n_sblk);
        up(d_act_win, ww, a.win, a.n_win);
        note(hipStreamSynchronize(s), "sync worklists");  // the host vectors go out of scope
    }

    // k_lin_lm<true> (the default since round 6): four waves per SIMD, the window's view constants, the landmark block's running sums and
    // the tail's inputs in LDS (kba_kernels.hip:lin_lm_block) - scalar loads of the view constants return out of order, so every use of
    // one waited for all of them (round 5: 550 -> 513 us per round of 4096 slots through LDS).  With the camera-side sums in their raw
    // form (kba_items.hpp:lin_cam_half0: the 3 x 6 pose Jacobian is never formed) the kernel needs 129 registers instead of 149, so the
    // fourth wave costs nothing else: 505 -> 495 us per round, bench line +0.7 % against three waves.
    // Batches whose windows have so many views that the copy would cost occupancy (> 48 KB of LDS per workgroup: more than ~16 views)
    // and KBA_LIN_VLDS=0 (read once; the tests) take <false>: scalar loads - same bits in both variants.
    int lin_lds_set = 0;  // dynamic LDS k_lin_lm<false> was allowed beyond the default 48 KB (k_lin_lm<true> never needs more)
    void launch_lin_lm(int grid, hipStream_t s, const BatchView& v, const int32_t* wl) {
        static const int want_vlds = std::getenv("KBA_LIN_VLDS") ? std::atoi(std::getenv("KBA_LIN_VLDS")) : 1;
        const bool vlds = want_vlds != 0 && lin_lm_lds_bytes(P.Vmax, true) <= 48 * 1024;
        const void* fn = vlds ? (const void*)k_lin_lm<true> : (const void*)k_lin_lm<false>;
        const int lds = lin_lm_lds_bytes(P.Vmax, vlds);
        lin_variant = vlds ? 1 : 0;
        if (lds > 48 * 1024 && lin_lds_set < lds) {  // (beyond the default dynamic-LDS limit: many views)
            note(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds), "hipFuncSetAttribute(k_lin_lm)");
            lin_lds_set = lds;
        }
        const BatchView* vp = &v;
        const SolveConsts* cp = &c;
        void* args[] = {(void*)vp, (void*)cp, (void*)&wl};
        note(hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, lds, s), "launch k_lin_lm");
    }

    void solve_init(int max_iter, int select) override {
        it_no = 0;
        first_lin = true;  // the next linearisation defines the Jacobi scaling (WinState::compute_scale)
        assemble_pending = false;  // (a solve that ended right behind a linearisation leaves nothing for the next one)
        full_lists();
        hipLaunchKernelGGL(k_solve_init, dim3(cdiv(P.n_win, 256)), dim3(256), 0, ctx->stream, bv, c, max_iter, select);
        LAUNCH_CHECK("k_solve_init");
    }

    // Event pair around one launch of a timed kernel (nullptr once the pool is exhausted).
    EventPair* timed(int kernel, hipStream_t on = nullptr) {
        if (ev_used >= 16384) return nullptr;
        if (ev_used == ev_pool.size()) {
            EventPair e;
            e.kernel = kernel;
            note(hipEventCreate(&e.a), "hipEventCreate");
            note(hipEventCreate(&e.b), "hipEventCreate");
            ev_pool.push_back(e);
        }
        EventPair* ep = &ev_pool[ev_used++];
        ep->kernel = kernel;
        note(hipEventRecord(ep->a, on ? on : ctx->stream), "hipEventRecord");
        return ep;
    }

    void linearize() override {
        hipStream_t s = ctx->stream;
        {
            if (P.TV) {
                hipLaunchKernelGGL(k_view_consts, dim3(cdiv(P.TV, 256)), dim3(256), 0, s, bv);
                LAUNCH_CHECK("k_view_consts");
            }
            // ground-plane rows first: the landmark pass adds them to the landmark blocks
            EventPair* ep = timed(LIMO_KERNEL_LINEARIZE);
            for (size_t i = 0; i < pv.size(); ++i)
                if (wl[i].cur.n_lblk) {
                    launch_lin_lm(wl[i].cur.n_lblk, s, pv[i], wl[i].cur.lblk);
                    LAUNCH_CHECK("k_lin_lm");
                }
            if (ep) note(hipEventRecord(ep->b, s), "hipEventRecord");
        }
        if (shard_P > 1) {
            for (size_t i = 0; i < pv.size(); ++i)
                if (wl[i].cur.n_win) {
                    hipLaunchKernelGGL(k_shard_reduce, dim3(wl[i].cur.n_win), dim3(kBlock), 0, s, pv[i], wl[i].cur.win, local_shards[i], 0);
                    LAUNCH_CHECK("k_shard_reduce");
                }
            // Sharded: the camera assembly only has to come before the Schur complement when it defines the Jacobi scale (the
            // first linearisation of a solve).  Every other iteration it waits for the slabs and ONE exchange serves both (step()).
            if (!first_lin) {
                assemble_pending = true;
                return;
            }
            first_lin = false;
            exchange(1);
        }
        assemble(it_no);
    }

    // k_cam_assemble + the active-window counter of iteration `iter`: a ring of 4 slots so the host can read iteration i-1
    // while iteration i runs
    void assemble(int iter) {
        hipStream_t s = ctx->stream;
        const int slot = iter & 3;
        BatchView bvs = bv;
        bvs.n_active = bv.n_active + 2 * slot;
        bvs.n_active_host = d_h_active + slot;
        const WorkLists& a = wl[0].cur;
        launch_cam_assemble(bvs, a.win, a.n_win, s);
        LAUNCH_CHECK("k_cam_assemble");
        note(hipEventRecord(act_ev[slot], s), "record n_active");
    }

    // Lagging by one iteration: the count of iteration i-1 is read while iteration i is already enqueued, so the
    // host never drains the stream inside a solve.  The price is at most one extra iteration of no-op launches.
    int active_count() override {
        if (rc != LIMO_OK) return 0;
        const int cur = it_no++;
        if (cur == 0) return P.n_win;  // iteration zero: nothing to wait for yet
        const int slot = (cur - 1) & 3;
        note(hipEventSynchronize(act_ev[slot]), "sync n_active");
        if (rc != LIMO_OK) return 0;
        const int a = h_active[slot], listed = wl[0].cur.n_win;
        static const bool trace = std::getenv("KBA_TRACE_ACTIVE") != nullptr;  // profiling aid
        if (trace) std::fprintf(stderr, "[kba] iteration %d: active %d, listed %d, span %d\n", cur - 1, a, listed, c.schur_span);
        // re-batch when at most half of the listed windows still iterate (and the list is worth shrinking)
        if (a > 0 && listed >= 8 && 2 * a <= listed) rebatch();
        return a;
    }

    void expire(int) override {
        if (assemble_pending) {  // sharded: the camera assembly of the last linearisation was deferred behind the Schur slabs - the
                                 // time cap ends the solve before them: assemble now (exchange of the linearisation sums only), so
                                 // that the windows' cost is the cost of the point they stop at
            assemble_pending = false;
            exchange(1);
            assemble(it_no - 1);
        }
        hipLaunchKernelGGL(k_expire, dim3(cdiv(P.n_win, 256)), dim3(256), 0, ctx->stream, bv);
        LAUNCH_CHECK("k_expire");
    }

    // The Schur kernels of one view over its three lists, in this order: both fast-class lists in ONE launch where the caller allows
    // the pair kernel (kba_kernels.hip:k_schur_lean_pair), else plain groups, then ground-plane groups; then the generic windows.
    // Ground-plane groups of a batch in which the pack found narrow ones (plan.narrow; SchurGroup::gp_class), where the records' spans
    // and packed slabs are in use: k_schur_lean_gp, and k_schur_lean_pair<2, 3, true> in a draining round - their waves run the
    // narrow tile or the three-panel tile as the record says.  KBA_SCHUR_GP_WIDE: the three-panel kernels, as in every other batch.
    void launch_schur(const BatchView& v, const int32_t* wl_plain, int n_plain, const int32_t* wl_fgp, int n_fgp, const int32_t* wl_gen, int n_gen, bool pair,
                      hipStream_t s) {
        int span = c.schur_span, span_gp = c.schur_span_gp, packed = c.slab_packed;
        const bool narrow = plan.narrow && !gp_wide && packed && span == kSchurSpan && span_gp == kSchurSpanGp;
        const bool wide = !narrow || P.n_sgrp_wide > 0;  // three-panel waves run
        if (pair) {
            void* args[] = {(void*)&v, (void*)&wl_plain, (void*)&n_plain, (void*)&wl_fgp, (void*)&span, (void*)&span_gp, (void*)&packed};
            note(hipLaunchKernel(narrow ? (const void*)k_schur_lean_pair<2, 3, true> : (const void*)k_schur_lean_pair<2, 3>, dim3(n_plain + n_fgp), dim3(64), args,
                                 std::max(plan.plain_lds, plan.leangp_lds), s),
                 "launch k_schur_lean_pair");
            ++n_pair_launches;
        }
        if (!pair && n_plain) {
            void* args[] = {(void*)&v, (void*)&wl_plain, (void*)&span, (void*)&span_gp, (void*)&packed};
            note(hipLaunchKernel(schur_fn_plain, dim3(n_plain), dim3(64), args, plan.plain_lds, s), "launch k_schur_lean");
        }
        if (!pair && n_fgp && narrow) {
            void* args[] = {(void*)&v, (void*)&wl_fgp};
            note(hipLaunchKernel(schur_fn_narrow, dim3(n_fgp), dim3(64), args, plan.leangp_lds, s), "launch k_schur_lean_gp");
        }
        if (!pair && n_fgp && !narrow) {
            void* args[] = {(void*)&v, (void*)&wl_fgp, (void*)&span, (void*)&span_gp, (void*)&packed};
            note(hipLaunchKernel(schur_fn_leangp, dim3(n_fgp), dim3(64), args, plan.leangp_lds, s), "launch k_schur_lean (gp)");
        }
        if (pair || n_fgp) {
            n_narrow_launches += narrow ? 1 : 0;
            n_widegp_launches += wide ? 1 : 0;
        }
        if (n_gen) {
            void* args[] = {(void*)&v, (void*)&wl_gen, (void*)&span, (void*)&span_gp};
            note(hipLaunchKernel(schur_fn_gen, dim3(n_gen), dim3(64 * kWideWaves), args, plan.wide_lds, s), "launch k_schur_wide");
        }
    }

    // ---- the other kernels of the train, ONE launch site each: block size, dynamic LDS and argument order are fixed here; view,
    // worklist, grid and stream are the caller's - the lock-step solve (linearize / assemble / step / trim) and the rounds of the
    // streaming solve (enqueue_round).  A grid of 0 launches nothing.
    void launch_cam_assemble(const BatchView& v, const int32_t* list, int grid, hipStream_t s) {
        if (!grid) return;
        // (grid: the windows the launch can list - the same bits from either form, so the form is this launch's own choice)
        const bool half = cam_lanes_for_launch(cam_plan.asm_half_ok, cam_plan.asm_resident, grid, cam_lanes_forced) == kCamLanesHalf;
        if (half)
            hipLaunchKernelGGL(k_cam_assemble<kCamLanesHalf>, dim3(grid), dim3(kCamLanesHalf), plan.asm_bytes, s, v, c, list);
        else
            hipLaunchKernelGGL(k_cam_assemble<kBlock>, dim3(grid), dim3(kBlock), plan.asm_bytes, s, v, c, list);
        ++n_cam_launches[0][half ? 0 : 1];
    }
    void launch_cam_solve(const BatchView& v, const int32_t* list, int grid, hipStream_t s) {
        if (!grid) return;
        const bool half = cam_lanes_for_launch(cam_plan.solve_half_ok, cam_plan.solve_resident, grid, cam_lanes_forced) == kCamLanesHalf;
        if (half)
            hipLaunchKernelGGL(k_cam_solve<kCamLanesHalf>, dim3(grid), dim3(kCamLanesHalf), plan.solve_bytes, s, v, c, list);
        else
            hipLaunchKernelGGL(k_cam_solve<kBlock>, dim3(grid), dim3(kBlock), plan.solve_bytes, s, v, c, list);
        ++n_cam_launches[1][half ? 0 : 1];
    }
    void launch_backsub(const BatchView& v, const int32_t* list, int grid, hipStream_t s) {
        if (grid) hipLaunchKernelGGL(k_backsub, dim3(grid), dim3(kBlock), 0, s, v, c, list);
    }
    void launch_step_decide(const BatchView& v, const int32_t* list, int grid, hipStream_t s) {
        if (grid) hipLaunchKernelGGL(k_step_decide, dim3(grid), dim3(64), 0, s, v, c, list);
    }
    void launch_after_step(const BatchView& v, const int32_t* list, int grid, hipStream_t s) {  // accepted landmarks, re-damping after a rejected step
        if (grid) hipLaunchKernelGGL(k_after_step, dim3(grid), dim3(kBlock), 0, s, v, c, list);
    }
    void launch_trim_residual(const BatchView& v, const int32_t* list, int grid, hipStream_t s) {
        if (grid) hipLaunchKernelGGL(k_trim_residual, dim3(grid), dim3(kBlock), 0, s, v, d_plane_rep, d_plane_dep, list);
    }
    // (grid: a lane per landmark of the batch in lock-step, a workgroup per counted landmark block in a streaming round)
    void launch_trim_max(const BatchView& v, int shard, int grid, hipStream_t s) {
        if (grid) hipLaunchKernelGGL(k_trim_max, dim3(grid), dim3(kBlock), 0, s, v, (const double*)d_plane_rep, (const double*)d_plane_dep, shard, shard_P);
    }
    void launch_trim_select(const BatchView& v, int grid, hipStream_t s) {
        if (grid) hipLaunchKernelGGL(k_trim_select, dim3(grid), dim3(kBlock), plan.trim_bytes, s, v, c);
    }

    void step() override {
        hipStream_t s = ctx->stream;
        if (c.slab_packed) spart_has_packed = true;
        const WorkLists& a = wl[0].cur;  // (the window list is the same for every view)
        {
            // (a step without Schur blocks - no window with a variable landmark - launches nothing and counts no launch)
            int n_schur = 0;
            for (size_t i = 0; i < pv.size(); ++i) n_schur += wl[i].cur.n_sblk;
            EventPair* ep = n_schur ? timed(LIMO_KERNEL_SCHUR) : nullptr;
            for (size_t i = 0; i < pv.size(); ++i) {
                const WorkLists& l = wl[i].cur;
                launch_schur(pv[i], l.sblk, l.n_sblk_plain, l.sblk + l.n_sblk_plain, l.n_sblk_fgp, l.sblk + l.n_sblk_plain + l.n_sblk_fgp,
                             l.n_sblk - l.n_sblk_plain - l.n_sblk_fgp, false, s);
                LAUNCH_CHECK("Schur kernels");
            }
            if (ep) note(hipEventRecord(ep->b, s), "hipEventRecord");
        }
        if (shard_P > 1) {
            if (a.n_win)
                for (size_t i = 0; i < pv.size(); ++i) {
                    hipLaunchKernelGGL(k_shard_reduce, dim3(a.n_win), dim3(kBlock), 0, s, pv[i], a.win, local_shards[i], 1);
                    hipLaunchKernelGGL(k_slab_reduce, dim3(a.n_win, 8), dim3(kBlock), 0, s, pv[i], a.win, shard_P);
                    LAUNCH_CHECK("k_slab_reduce");
                }
            if (assemble_pending) {  // ONE exchange: camera-side sums + ground-plane blocks + scalars + [S | rhs]
                assemble_pending = false;
                exchange(3);
                assemble(it_no - 1);  // (active_count() has moved it_no on to the next iteration)
            } else {
                exchange(2);
            }
        }
        launch_cam_solve(bv, a.win, a.n_win, s);
        LAUNCH_CHECK("k_cam_solve");
        for (size_t i = 0; i < pv.size(); ++i) {
            launch_backsub(pv[i], wl[i].cur.lblk, wl[i].cur.n_lblk, s);
            LAUNCH_CHECK("k_backsub");
        }
        if (shard_P > 1 && a.n_win)
            for (size_t i = 0; i < pv.size(); ++i) {
                hipLaunchKernelGGL(k_shard_reduce, dim3(a.n_win), dim3(kBlock), 0, s, pv[i], a.win, local_shards[i], 2);
                LAUNCH_CHECK("k_shard_reduce");
            }
        exchange(4);
        launch_step_decide(bv, a.win, a.n_win, s);
        LAUNCH_CHECK("k_step_decide");
        for (size_t i = 0; i < pv.size(); ++i) {  // a rejected step: its landmark blocks are damped again for the next iteration
            launch_after_step(pv[i], wl[i].cur.lblk, wl[i].cur.n_lblk, s);
            LAUNCH_CHECK("k_after_step");
        }
    }

    void trim() override {
        hipStream_t s = ctx->stream;
        bool any = false;
        for (const WinDesc& d : P.win) any = any || d.do_trim;
        if (!any) return;
        for (size_t i = 0; i < pv.size(); ++i) {
            launch_trim_residual(pv[i], wl[i].full.blk, wl[i].full.n_blk, s);
            LAUNCH_CHECK("k_trim_residual");
        }
        for (size_t i = 0; i < pv.size(); ++i) {
            launch_trim_max(pv[i], local_shards[i], cdiv(P.TL, kBlock), s);
            LAUNCH_CHECK("k_trim_max");
        }
        exchange_trim();
        launch_trim_select(bv, P.n_win, s);
        LAUNCH_CHECK("k_trim_select");
    }

    // ------------------------------------------------------------------------------------------ streaming solve
    // Slot groups: the slots are split into `n_groups` groups, each with its own stream, worklists and scheduler state;
    // they take their windows from one shared cursor.  The groups run the same round sequence out of phase, so the
    // MFMA-bound Schur kernels and the latency-bound window-level kernels of one group overlap with the HBM-bound
    // scans of the other.
    struct StreamGroup {
        hipStream_t stream = nullptr, trim_stream = nullptr;
        bool own_stream = false;
        hipEvent_t sched_ev = nullptr, trim_ev = nullptr, done_ev = nullptr, round_ev[4] = {nullptr, nullptr, nullptr, nullptr};
        int32_t *d_slot_win = nullptr, *d_lists = nullptr, *d_slot_cnt = nullptr;
        int32_t *h_done = nullptr, *d_h_done = nullptr;  // pinned ring of 4
        int n_slots = 0;
        int cap[SL_COUNT] = {0};
        int mx[SL_COUNT] = {0};  // entries of list k a single window can have
        BatchView sv;
    };
    std::vector<StreamGroup> groups;
    int stream_groups_built = 0;
    hipEvent_t start_ev = nullptr;

    void stream_teardown() {
        for (StreamGroup& g : groups) {
            if (g.own_stream && g.stream) (void)hipStreamDestroy(g.stream);
            if (g.trim_stream) (void)hipStreamDestroy(g.trim_stream);
            for (hipEvent_t e : {g.sched_ev, g.trim_ev, g.done_ev, g.round_ev[0], g.round_ev[1], g.round_ev[2], g.round_ev[3]})
                if (e) (void)hipEventDestroy(e);
            if (g.h_done) ctx->host_free(g.h_done, 64);
        }
        groups.clear();
        if (start_ev) (void)hipEventDestroy(start_ev);
        start_ev = nullptr;
    }

    // Streams, events, lists and scheduler state of the slot groups of `geo` (kba_batch_plan.hpp:stream_geometry), kept for the
    // re-solves of the batch while the number of groups stays (the rest of the geometry is fixed by the batch).
    int stream_setup(const StreamGeometry& geo) {
        const int n_groups = geo.n_groups;
        if (stream_groups_built == n_groups) return LIMO_OK;
        (void)hipStreamSynchronize(ctx->stream);
        stream_teardown();  // (device blocks of an earlier layout stay with the batch until it is destroyed)
        n_slots = geo.n_slots;
        if (!d_sched_ctl && dmalloc((void**)&d_sched_ctl, sizeof(int32_t) * 8)) return LIMO_ERR_RUNTIME;
        HIP_TRY(ctx, hipEventCreateWithFlags(&start_ev, hipEventDisableTiming));
        groups.resize(n_groups);
        for (int gi = 0; gi < n_groups; ++gi) {
            StreamGroup& g = groups[gi];
            g.n_slots = geo.group_slots[gi];
            g.sv = bv;
            size_t total = 0;
            for (int k = 0; k < SL_COUNT; ++k) {
                g.mx[k] = geo.mx[k];
                g.cap[k] = g.n_slots * g.mx[k];
                g.sv.sched_off[k] = (int32_t)total;
                total += 1 + (size_t)std::max(1, g.cap[k]);
            }
            if (dmalloc((void**)&g.d_lists, sizeof(int32_t) * total)) return LIMO_ERR_RUNTIME;
            if (dmalloc((void**)&g.d_slot_win, sizeof(int32_t) * std::max(1, g.n_slots))) return LIMO_ERR_RUNTIME;
            if (dmalloc((void**)&g.d_slot_cnt, sizeof(int32_t) * (SL_COUNT + 1) * std::max(1, g.n_slots))) return LIMO_ERR_RUNTIME;
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
        stream_groups_built = n_groups;
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
    void enqueue_round(StreamGroup& g, int round, bool time_kernels, int in_flight_max) {
        hipStream_t s = g.stream;
        const BatchView& sv = g.sv;
        int cap[SL_COUNT];
        const int bound = std::max(1, std::min(g.n_slots, in_flight_max));
        for (int k = 0; k < SL_COUNT; ++k) cap[k] = std::min(g.cap[k], bound * g.mx[k]);
        auto L = [&](int k) { return (const int32_t*)(g.d_lists + sv.sched_off[k] + 1); };
        if (round > 0) note(hipStreamWaitEvent(s, g.trim_ev, 0), "wait trim");  // last round's trimming re-armed its windows
        hipLaunchKernelGGL(k_sched_advance, dim3(cdiv(g.n_slots, 256)), dim3(256), 0, s, sv, c);
        hipLaunchKernelGGL(k_sched_scan, dim3(1), dim3(kSchedThreads), 0, s, sv, round);
        hipLaunchKernelGGL(k_sched_fill, dim3(cdiv(g.n_slots, 4)), dim3(256), 0, s, sv, c);
        LAUNCH_CHECK("scheduler kernels");
        // ---- trimming of the windows whose trimming solve just ended, on the side stream: k_trim_select is a
        //      latency-bound sort (one workgroup per window, ~0.3 ms) - the other windows iterate meanwhile, the
        //      trimmed ones join again in the next round (k_trim_select arms their next solve)
        note(hipEventRecord(g.sched_ev, s), "record sched");
        note(hipStreamWaitEvent(g.trim_stream, g.sched_ev, 0), "wait sched");
        launch_trim_residual(sv, L(SL_TBLK), cap[SL_TBLK], g.trim_stream);
        launch_trim_max(sv, 0, cap[SL_TLBLK], g.trim_stream);
        launch_trim_select(sv, cap[SL_TWIN], g.trim_stream);
        LAUNCH_CHECK("trim kernels");
        note(hipEventRecord(g.trim_ev, g.trim_stream), "record trim");
        // ---- linearisation of the windows that need it (their per-view constants: k_sched_fill above)
        {
            EventPair* ep = time_kernels ? timed(LIMO_KERNEL_LINEARIZE, s) : nullptr;
            if (cap[SL_LBLK]) launch_lin_lm(cap[SL_LBLK], s, sv, L(SL_LBLK));
            if (ep) note(hipEventRecord(ep->b, s), "hipEventRecord");
        }
        launch_cam_assemble(sv, L(SL_WIN), cap[SL_WIN], s);
        LAUNCH_CHECK("linearisation kernels");
        // ---- trust-region step of the windows that iterate
        {
            EventPair* ep = time_kernels && (cap[SL_SPLAIN] || cap[SL_SFGP] || cap[SL_SGEN]) ? timed(LIMO_KERNEL_SCHUR, s) : nullptr;
            // few windows in flight (the batch drains): both fast-class lists in one launch (kba_kernels.hip:k_schur_lean_pair)
            const bool pair = schur_pair_ok && bound <= kSchurPairBound && cap[SL_SPLAIN] && cap[SL_SFGP];
            launch_schur(sv, L(SL_SPLAIN), cap[SL_SPLAIN], L(SL_SFGP), cap[SL_SFGP], L(SL_SGEN), cap[SL_SGEN], pair, s);
            if (ep) note(hipEventRecord(ep->b, s), "hipEventRecord");
        }
        launch_cam_solve(sv, L(SL_WIN), cap[SL_WIN], s);
        launch_backsub(sv, L(SL_LBLK), cap[SL_LBLK], s);
        launch_step_decide(sv, L(SL_WIN), cap[SL_WIN], s);
        launch_after_step(sv, L(SL_LBLK), cap[SL_LBLK], s);
        LAUNCH_CHECK("step kernels");
        note(hipEventRecord(g.round_ev[round & 3], s), "record round");
    }

    // ---- a whole solve in ONE launch: k_solve_wg (a workgroup per window) and k_solve_coop (G workgroups per window that meet at
    // device-wide barriers).  Which solve takes them: kba_batch_plan.hpp:choose_solve_path.
    long long cap_ticks() const { return opts.max_solver_time_sec > 0.0 ? std::max(1ll, (long long)(opts.max_solver_time_sec * 1e8)) : 0ll; }
    void solve_wg() {
        const int lds = plan.onelaunch_lds;
        note(hipFuncSetAttribute((const void*)k_solve_wg, hipFuncAttributeMaxDynamicSharedMemorySize, lds), "hipFuncSetAttribute(k_solve_wg)");
        hipLaunchKernelGGL(k_solve_wg, dim3(P.n_win), dim3(kBlock), lds, ctx->stream, bv, c, cap_ticks(), d_plane_rep, d_plane_dep);
        LAUNCH_CHECK("k_solve_wg");
    }

    int32_t* d_coop_bar = nullptr;
    double* d_coop_red = nullptr;
    bool coop_launched = false;
    // false: the launch was refused (nothing ran) - the caller takes the lock-step path
    bool solve_coop(const CoopGeometry& geo, const SolveSwitches& sw) {
        const int lds = coop_lds_bytes(plan);
        if (!d_coop_bar && dmalloc((void**)&d_coop_bar, sizeof(int32_t) * 8 * P.n_win)) return false;
        if (!d_coop_red && dmalloc((void**)&d_coop_red, sizeof(double) * kCoopRedStride * P.n_win)) return false;
        if (hipFuncSetAttribute((const void*)k_solve_coop, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        note(hipMemsetAsync(d_coop_bar, 0, sizeof(int32_t) * 8 * P.n_win, ctx->stream), "memset barrier words");
        if (spart_has_packed) {
            note(hipMemsetAsync(bv.S_part, 0, sizeof(double) * (size_t)std::max<int64_t>(1, P.spart_total), ctx->stream), "clear packed Schur slabs");
            spart_has_packed = false;
        }
        h_active[8] = 0;
        CoopParams cp;
        cp.G = geo.G;
        cp.vp = plan.plain_tm;
        cp.vg = plan.gp_tm;
        cp.schur_lds = plan.schur_wave_lds / (int)sizeof(double);
        cp.cap_ticks = cap_ticks();
        // barrier timeout in ticks of the 100 MHz constant clock (KBA_COOP_TIMEOUT_MS=0: give up at the first wait - how the tests
        // reach the recovery path of limo_ba_batch_solve)
        // default 50 ms (the whole call is ~5 ms; the longest phase between two barriers - the quantile trimming - well under 1 ms):
        // a barrier that is not met by then is lost, and the caller of a 10 Hz pipeline should not wait seconds to learn it
        cp.timeout_ticks = std::max(0ll, (long long)(sw.coop_timeout_ms * 1e5));
        cp.bar = d_coop_bar;
        cp.abort_host = d_h_active + 8;
        cp.plane_rep = d_plane_rep;
        cp.plane_dep = d_plane_dep;
        cp.red = d_coop_red;
        SolveConsts cc = c;
        cc.slab_packed = 0;  // (tile layout: the slab sum of k_solve_coop indexes it)
        void* args[] = {(void*)&bv, (void*)&cc, (void*)&cp};
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

    // The host only enqueues; it learns that all windows are done from a pinned word the scheduler writes, two rounds
    // late (so the streams never drain inside a solve).
    int solve_streaming(const SolveSwitches& sw) {
        if (stream_setup(stream_geometry(P, {c.schur_span, c.schur_span_gp}, sw)) != LIMO_OK) return LIMO_ERR_RUNTIME;
        if (c.slab_packed) spart_has_packed = true;
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
            ++n_rounds;
            if (sched_trace) enq_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enq0).count();
            if (rc != LIMO_OK) break;
            if (round >= kLag) {
                finished = true;
                for (StreamGroup& g : groups) {
                    note(hipEventSynchronize(g.round_ev[(round - kLag) & 3]), "sync round");
                    if (rc != LIMO_OK) break;
                    const int d = g.h_done[(round - kLag) & 3];
                    if (d < P.n_win) finished = false;
                    done_seen = std::max(done_seen, d);
                }
                if (sched_trace) done_curve.push_back(groups[0].h_done[(round - kLag) & 3]);
            }
            if (round > 200000) {
                rc = LIMO_ERR_RUNTIME;
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
            note(hipStreamWaitEvent(g.stream, g.trim_ev, 0), "wait trim");
            if (g.stream != s0) {
                note(hipEventRecord(g.done_ev, g.stream), "record done");
                note(hipStreamWaitEvent(s0, g.done_ev, 0), "wait group");
            }
        }
        return rc;
    }

    // An evaluation of an evaluate-only batch: the per-view constants + the materialised pass, on the context's stream.
    void launch_evaluate(int apply_loss, double* d_cost, uint8_t* d_valid) {
        hipLaunchKernelGGL(k_view_consts_all, dim3(cdiv(P.TV, 256)), dim3(256), 0, ctx->stream, bv);
        hipLaunchKernelGGL(k_evaluate, dim3(evaluate_grid(P.n_echunk)), dim3(kBlock), 0, ctx->stream, bv, c, apply_loss, d_cost, d_valid);
    }

    int collect_linearize_events() {
        if (ev_used) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (size_t i = 0; i < ev_used; ++i) {
                float ms = 0.f;
                HIP_TRY(ctx, hipEventElapsedTime(&ms, ev_pool[i].a, ev_pool[i].b));
                k_ms_acc[ev_pool[i].kernel] += ms;
                k_launches[ev_pool[i].kernel] += 1;
            }
            ev_used = 0;
        }
        return LIMO_OK;
    }
};

// =============================================================================================== C-ABI
extern "C" {

int limo_abi_version(void) {
    return LIMO_ABI_VERSION;
}

int limo_ctx_create(int device, limo_ctx** out) {
    if (!out) return LIMO_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return LIMO_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return LIMO_ERR_NO_DEVICE;
    limo_ctx* c = new limo_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return LIMO_ERR_RUNTIME;
    }
    c->stream = c->own;
    *out = c;
    return LIMO_OK;
}

void* limo_host_alloc(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1) == hipSuccess ? p : nullptr;
}
void limo_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

void limo_ctx_destroy(limo_ctx* ctx) {
    if (!ctx) return;
    if (ctx->depth_ws && ctx->depth_ws_free) ctx->depth_ws_free(ctx->depth_ws);
    if (ctx->comm) (void)ncclCommDestroy((ncclComm_t)ctx->comm);
    ctx->pool_release();
    if (ctx->own) (void)hipStreamDestroy(ctx->own);
    delete ctx;
}

int limo_ctx_set_stream(limo_ctx* ctx, void* hip_stream) {
    if (!ctx) return LIMO_ERR_INVALID;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own;
    return LIMO_OK;
}

const char* limo_last_error(const limo_ctx* ctx) {
    return ctx ? ctx->err.c_str() : "null context";
}

void limo_ba_default_options(limo_ba_options* o) {
    if (!o) return;
    o->depth_thres = 0.16;
    o->reprojection_thres = 1.6;
    o->depth_quantile = 0.95;
    o->reprojection_quantile = 0.95;
    o->num_trim_rounds = 1;
    o->trim_solver_iterations = 2;
    o->min_landmarks_for_trimming = 100;
    o->minimum_number_residual_groups = 30;
    o->max_num_iterations = 100;
    o->max_solver_time_sec = -1.0;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->min_relative_decrease = 1e-3;
    o->max_num_consecutive_invalid_steps = 5;
    o->jacobi_scaling = 1;
}

static int batch_create_impl(limo_ctx* ctx, int32_t n, const limo_ba_window* windows, const limo_ba_options* opts,
                             const PackOptions& po, limo_ba_batch** out, bool shards_are_ranks = false) {
    if (!ctx || !out) return LIMO_ERR_INVALID;
    *out = nullptr;
    limo_ba_options o;
    if (opts)
        o = *opts;
    else
        limo_ba_default_options(&o);
    if (po.shards > 1 && n != 1) {  // (what the lock-step solve relies on: a sharded batch never re-batches, limo_ba_batch::rebatch)
        ctx->err = "a landmark-sharded batch holds exactly one window";
        return LIMO_ERR_INVALID;
    }
    std::unique_ptr<limo_ba_batch> b(new limo_ba_batch());
    b->ctx = ctx;
    b->opts = o;
    const auto t_c0 = std::chrono::steady_clock::now();
    // Large batches pack into the context's pinned arena when no other live batch holds it (limo_ctx.hpp:pack_arena).  The first large
    // batch of a context only measures what it would have needed; the arena is made right behind its packing, for the next one.
    PackArena lend;
    const bool lending = n >= 128 && !ctx->pack_arena_busy && hipSetDevice(ctx->device) == hipSuccess;
    auto arena_resize = [&](size_t wanted) {  // (only while no batch holds the arena)
        const size_t step = size_t(64) << 20;
        const size_t cap = std::min(limo_ctx::kPackArenaMax, (wanted + wanted / 8 + step - 1) / step * step);
        if (cap <= ctx->pack_arena.cap) return;
        if (ctx->pack_arena.p) pack_arena_register(ctx->pack_arena.p, ctx->pack_arena.cap, false);
        if (ctx->pack_arena.ensure(cap) == hipSuccess)
            pack_arena_register(ctx->pack_arena.p, cap, true);
        else
            (void)hipGetLastError();
    };
    if (lending) {
        if (ctx->pack_arena.p && ctx->pack_arena_wanted > ctx->pack_arena.cap) arena_resize(ctx->pack_arena_wanted);  // the last batch did not fit
        lend.base = static_cast<char*>(ctx->pack_arena.p);
        lend.cap = ctx->pack_arena.cap;
    }
    int rc = LIMO_OK;
    try {  // (the pack's host threads hand their exceptions to the caller, kba_pack.cpp:PackPool - none may cross the C ABI)
        PackArenaLend loan(lending ? &lend : nullptr);
        PackOptions pod = po;
        pod.host_pair_planes = false;  // (k_pair_fill forms the planes on the device: limo_ba_batch::upload)
        rc = pack_windows(n, windows, o, pod, b->P, ctx->err);
    } catch (const std::bad_alloc&) {
        ctx->err = "pack_windows: out of host memory";
        return LIMO_ERR_RUNTIME;
    } catch (const std::exception& e) {
        ctx->err = std::string("pack_windows: ") + e.what();
        return LIMO_ERR_RUNTIME;
    }
    if (lending) {
        ctx->pack_arena_wanted = std::max(ctx->pack_arena_wanted, lend.wanted);
        if (lend.used > 0) {
            ctx->pack_arena_busy = true;
            b->holds_pack_arena = true;
        } else if (!ctx->pack_arena.p && lend.wanted > 0) {
            arena_resize(lend.wanted);  // the first large batch of the context: ready for the next one
        }
    }
    const auto t_c1 = std::chrono::steady_clock::now();
    if (rc == LIMO_OK) {
        if (hipSetDevice(ctx->device) != hipSuccess) rc = LIMO_ERR_NO_DEVICE;
    }
    b->pose_batch = po.per_window_prior;
    b->shard_P = b->P.n_shards;
    b->shard_virtual = !shards_are_ranks;
    b->shard_rank = shards_are_ranks ? ctx->comm_rank : 0;
    if (b->shard_P > 1) {  // shard s lives on rank s mod world (all of them here when there is no communicator)
        const int world = shards_are_ranks ? ctx->comm_world : 1, me = shards_are_ranks ? ctx->comm_rank : 0;
        for (int r = 0; r < b->shard_P; ++r)
            if (r % world == me) b->local_shards.push_back(r);
        if (b->local_shards.size() > 8) {
            ctx->err = "at most 8 shards per GPU";
            return LIMO_ERR_INVALID;
        }
    } else {
        b->local_shards.push_back(0);
    }
    b->c = b->consts_for(o);
    if (rc == LIMO_OK) rc = b->upload();
    if (std::getenv("KBA_PACK_TRACE"))
        std::fprintf(stderr, "[kba] create: pack %.1f ms, upload %.1f ms\n", std::chrono::duration<double, std::milli>(t_c1 - t_c0).count(),
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_c1).count());
    if (rc != LIMO_OK) return rc;
    *out = b.release();
    return LIMO_OK;
}

int limo_ba_batch_create(limo_ctx* ctx, int32_t n_windows, const limo_ba_window* windows, limo_ba_batch** out) {
    // min_landmarks_for_trimming decides do_trim at pack time; take it from the default options here and
    // refresh at solve() if the caller passes different options.
    return batch_create_impl(ctx, n_windows, windows, nullptr, PackOptions(), out);
}

int limo_ba_batch_solve(limo_ba_batch* b, const limo_ba_options* opts) {
    if (!b) return LIMO_ERR_INVALID;
    limo_ctx* ctx = b->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;
    if (opts) {
        if (opts->min_landmarks_for_trimming != b->opts.min_landmarks_for_trimming) {
            for (int w = 0; w < b->P.n_win; ++w) b->P.win[w].do_trim = b->P.win[w].n_lm > opts->min_landmarks_for_trimming;
            if (b->shard_P > 1) {  // (the consumer view of a sharded batch carries its own descriptors: both copies follow)
                const std::vector<WinDesc> wc = exchange_consumer_windows(b->P);
                HIP_TRY(ctx, hipMemcpy((void*)b->d_win_orig, b->P.win.data(), sizeof(WinDesc) * b->P.n_win, hipMemcpyHostToDevice));
                HIP_TRY(ctx, hipMemcpy((void*)b->bv.win, wc.data(), sizeof(WinDesc) * b->P.n_win, hipMemcpyHostToDevice));
            } else {
                HIP_TRY(ctx, hipMemcpyAsync((void*)b->bv.win, b->P.win.data(), sizeof(WinDesc) * b->P.n_win, hipMemcpyHostToDevice,
                                            ctx->stream));
            }
        }
        b->opts = *opts;
        b->c = b->consts_for(*opts);
    }
    b->rc = LIMO_OK;
    // iteration log: every solve starts its windows' logs at zero entries (not offered for a landmark-sharded batch)
    if (b->bind_log(ctx->iteration_log && b->shard_P == 1) != LIMO_OK) return LIMO_ERR_RUNTIME;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(ctx, hipEventRecord(b->ev_total_a, ctx->stream));
    // Which path (kba_batch_plan.hpp:choose_solve_path; the KBA_* switches are read per call: the tests switch paths).  All paths
    // give the same bits.
    const SolveSwitches sw = read_solve_switches();
    SolveFacts facts;
    facts.max_solver_time_sec = b->opts.max_solver_time_sec;
    facts.shard_P = b->shard_P;
    facts.pose_batch = b->pose_batch;
    facts.pristine = b->pristine;
    facts.coop_strikes = ctx->coop_strikes;
    facts.coop_benched = ctx->coop_benched;
    const SolveChoice ch = choose_solve_path(b->P, b->plan, sw, facts);
    if (ch.benched) ++ctx->coop_benched;
    b->n_rounds = b->n_pair_launches = b->n_narrow_launches = b->n_widegp_launches = 0;
    b->gp_wide = sw.gp_wide;
    b->cam_lanes_forced = sw.cam_lanes;
    b->n_cam_launches[0][0] = b->n_cam_launches[0][1] = b->n_cam_launches[1][0] = b->n_cam_launches[1][1] = 0;
    b->lin_variant = 1;
    long long* info = ctx->last_solve_info;
    std::fill(info, info + 8, 0ll);
    auto launch_sequence = [&]() {
        info[0] = ch.fallback;
        if (ch.fallback == PATH_STREAMING)
            b->solve_streaming(sw);
        else
            run_schedule(*b, b->opts);
    };
    switch (ch.path) {
        case PATH_WG:
            info[0] = PATH_WG;
            b->solve_wg();
            break;
        case PATH_COOP:
            if (b->solve_coop(ch.coop, sw)) {
                info[0] = PATH_COOP;
                info[2] = ch.coop.G;
                ctx->coop_benched = 0;
                break;
            }
            [[fallthrough]];  // the launch was refused (nothing ran)
        default:
            launch_sequence();
    }
    b->pristine = false;
    if (b->coop_launched) {
        // A device-wide barrier of k_solve_coop that was not met in time aborts the launch (kba_kernels.hip:coop_sync) and leaves
        // poses, landmarks and LM state half-updated.  That is recoverable: the batch's initial state is restored (the pristine
        // copies limo_ba_batch_reset uses) and the same windows go through the launch sequence - same results, bit for bit.
        b->coop_launched = false;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (b->h_active[8] == 0) ctx->coop_strikes = 0;
        if (b->h_active[8] != 0) {
            b->h_active[8] = 0;
            info[1] = 1;
            ++ctx->coop_fallbacks;
            ++ctx->coop_strikes;
            if (b->reset_state() != LIMO_OK) return LIMO_ERR_RUNTIME;
            b->rc = LIMO_OK;
            launch_sequence();
            b->pristine = false;
        }
    }
    if (b->shard_P > 1 && !b->shard_virtual) {  // every rank ends with every landmark: sum of "owned, else zero"
        hipLaunchKernelGGL(k_lm_owned, dim3(cdiv(b->P.TL, 256)), dim3(256), 0, ctx->stream, b->bv, b->d_lm_tmp, b->shard_rank, b->shard_P,
                           ctx->comm_world);
        if (ctx->xfn) {
            b->host_exchange(b->d_lm_tmp, b->bv.lm, (size_t)3 * b->P.TL, 1);
            if (b->rc != LIMO_OK) return b->rc;
        } else {
            const ncclResult_t r = ncclAllReduce(b->d_lm_tmp, b->bv.lm, (size_t)3 * b->P.TL, ncclDouble, ncclSum, (ncclComm_t)ctx->comm, ctx->stream);
            b->note_nccl(r, "ncclAllReduce(landmarks)");
            if (r != ncclSuccess) return b->rc;
        }
        ++b->n_exchanges;
        b->exchange_bytes += (int64_t)sizeof(double) * 3 * b->P.TL;
    }
    if (info[0] == PATH_STREAMING) {
        info[3] = (long long)b->groups.size();
        info[4] = b->n_slots;
    }
    info[5] = b->n_rounds;
    info[6] = b->n_pair_launches;
    info[7] = b->lin_variant;
    ctx->last_schur_gp_info[0] = b->P.n_sgrp_narrow;
    ctx->last_schur_gp_info[1] = b->P.n_sgrp_wide;
    ctx->last_schur_gp_info[2] = b->n_narrow_launches;
    ctx->last_schur_gp_info[3] = b->n_widegp_launches;
    {
        long long* ci = ctx->last_cam_lanes_info;
        ci[0] = b->n_cam_launches[0][0];
        ci[1] = b->n_cam_launches[0][1];
        ci[2] = b->n_cam_launches[1][0];
        ci[3] = b->n_cam_launches[1][1];
        ci[4] = b->cam_occ.asm_half;
        ci[5] = b->cam_occ.asm_full;
        ci[6] = b->cam_occ.solve_half;
        ci[7] = b->cam_occ.solve_full;
        ci[8] = 0;
        for (const WinDesc& d : b->P.win) ci[8] += d.cam_scr_off >= 0 ? 1 : 0;
    }
    HIP_TRY(ctx, hipEventRecord(b->ev_total_b, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, b->ev_total_a, b->ev_total_b));
    b->total_ms_acc += ms;
    b->last_solve_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return b->rc;
}

int limo_ba_batch_reset(limo_ba_batch* b) {
    if (!b) return LIMO_ERR_INVALID;
    if (hipSetDevice(b->ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;
    return b->reset_state();
}

int limo_ba_batch_download(limo_ba_batch* b, limo_ba_window* windows_out, limo_ba_report* reports) {
    if (!b) return LIMO_ERR_INVALID;
    limo_ctx* ctx = b->ctx;
    const PackedBatch& P = b->P;
    std::vector<double> pose_v, pdir_v, pdist_v, lm_v;
    std::vector<WinState> st_v;
    const double *pose = nullptr, *pdir = nullptr, *pdist = nullptr, *lm = nullptr;
    const WinState* st = nullptr;
    {
        // [st | pose | pdir | pdist | lm] are neighbours in the batch's device block (kba_buffers.hpp order, upload()):
        // a small batch comes back with ONE copy into the context's pinned staging buffer instead of five into pageable
        // vectors (each of those is a blocking staged copy inside the runtime).
        const char* lo = reinterpret_cast<const char*>(b->bv.st);
        const char* hi = reinterpret_cast<const char*>(b->bv.lm) + sizeof(double) * 3 * (size_t)P.TL;
        auto inside = [&](const void* q) { return reinterpret_cast<const char*>(q) >= lo && reinterpret_cast<const char*>(q) < hi; };
        // A LARGE batch takes the same single copy through a pinned buffer the context keeps for it (grow-only, up to kBigStageMax):
        // five copies into fresh pageable vectors were staged by the runtime and paid their page faults - 6 of the 10 ms a
        // 1024-window download took.
        const bool neighbours = hi > lo && inside(b->bv.pose) && inside(b->bv.pdir) && inside(b->bv.pdist) && (P.TL == 0 || inside(b->bv.lm));
        const size_t span = neighbours ? (size_t)(hi - lo) : 0;
        void* hbuf = nullptr;
        if (neighbours && span <= ctx->staging.cap && ctx->staging.p) {
            hbuf = ctx->staging.p;
        } else if (neighbours && span <= limo_ctx::kBigStageMax) {
            if (ctx->staging_big.ensure(span, span + span / 4, limo_ctx::kBigStageMax) == hipSuccess)
                hbuf = ctx->staging_big.p;
            else
                (void)hipGetLastError();  // (no pinned memory to be had: the pageable path below)
        }
        if (hbuf) {
            HIP_TRY(ctx, hipMemcpyAsync(hbuf, lo, span, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            const char* h = static_cast<const char*>(hbuf);
            auto at = [&](const void* q) { return h + (reinterpret_cast<const char*>(q) - lo); };
            st = reinterpret_cast<const WinState*>(at(b->bv.st));
            pose = reinterpret_cast<const double*>(at(b->bv.pose));
            pdir = reinterpret_cast<const double*>(at(b->bv.pdir));
            pdist = reinterpret_cast<const double*>(at(b->bv.pdist));
            lm = reinterpret_cast<const double*>(at(b->bv.lm));
        } else {
            pose_v.resize((size_t)P.TK * 7);
            pdir_v.resize((size_t)P.TK * 3);
            pdist_v.resize(P.TK);
            lm_v.resize((size_t)P.TL * 3);
            st_v.resize(P.n_win);
            HIP_TRY(ctx, hipMemcpyAsync(pose_v.data(), b->bv.pose, sizeof(double) * pose_v.size(), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(pdir_v.data(), b->bv.pdir, sizeof(double) * pdir_v.size(), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(pdist_v.data(), b->bv.pdist, sizeof(double) * pdist_v.size(), hipMemcpyDeviceToHost, ctx->stream));
            if (P.TL) HIP_TRY(ctx, hipMemcpyAsync(lm_v.data(), b->bv.lm, sizeof(double) * lm_v.size(), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(st_v.data(), b->bv.st, sizeof(WinState) * st_v.size(), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            pose = pose_v.data();
            pdir = pdir_v.data();
            pdist = pdist_v.data();
            lm = lm_v.data();
            st = st_v.data();
        }
    }
    if (windows_out)
        for (int w = 0; w < P.n_win; ++w)
            if (windows_out[w].n_kf != P.win[w].n_kf || windows_out[w].n_lm != P.win[w].n_lm) {
                ctx->err = "download: window shape differs from create()";
                return LIMO_ERR_INVALID;
            }
    // windows are independent (every window writes its own arrays): host threads share them when the batch is large
    auto one_window = [&](int w) {
        const WinDesc& d = P.win[w];
        if (windows_out) {
            limo_ba_window& W = windows_out[w];
            std::memcpy(W.kf_pose, pose + 7 * (size_t)d.kf0, sizeof(double) * 7 * d.n_kf);
            std::memcpy(W.kf_plane_dir, pdir + 3 * (size_t)d.kf0, sizeof(double) * 3 * d.n_kf);
            std::memcpy(W.kf_plane_dist, pdist + d.kf0, sizeof(double) * d.n_kf);
            for (int l = 0; l < d.n_lm; ++l)  // packed order -> the caller's landmark order
                std::memcpy(W.lm_pos + 3 * (size_t)P.lm_id[d.lm0 + l], lm + 3 * (size_t)(d.lm0 + l), sizeof(double) * 3);
        }
        if (reports) {
            limo_ba_report& r = reports[w];
            const WinState& s = st[w];
            std::memset(&r, 0, sizeof(r));
            r.termination = s.term;
            r.num_solves = s.acc_solves;
            r.iterations_total = s.acc_iters;
            r.iterations_final = s.last_iters;
            r.successful_steps = s.acc_success;
            r.n_depth_blocks = d.n_depth;
            r.n_repr_blocks = d.n_repr;
            r.n_gp_blocks = d.n_gp;
            r.n_trimmed_landmarks = s.n_trimmed;
            r.num_linearizations = s.acc_lin;
            r.initial_cost = s.first_initial_cost;
            r.final_cost = s.solve_final_cost;
            r.time_sec = b->last_solve_sec;
        }
    };
    unsigned nt = std::min({std::thread::hardware_concurrency(), 32u, (unsigned)(P.n_win / 32)});
    if (const char* e = std::getenv("KBA_PACK_THREADS")) nt = (unsigned)std::max(1, std::atoi(e));
    if (nt <= 1) {
        for (int w = 0; w < P.n_win; ++w) one_window(w);
    } else {
        std::atomic<int> next{0};
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nt; ++t)
            pool.emplace_back([&] {
                for (int w0 = next.fetch_add(8); w0 < P.n_win; w0 = next.fetch_add(8))
                    for (int w = w0; w < std::min(w0 + 8, (int)P.n_win); ++w) one_window(w);
            });
        for (auto& th : pool) th.join();
    }
    return LIMO_OK;
}

int limo_ba_batch_trimmed(limo_ba_batch* b, int32_t w, uint8_t* removed) {
    if (!b || !removed || w < 0 || w >= b->P.n_win) return LIMO_ERR_INVALID;
    limo_ctx* ctx = b->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;
    const WinDesc& d = b->P.win[w];
    std::vector<uint8_t> st((size_t)std::max(1, (int)d.n_lm));
    if (d.n_lm) {
        HIP_TRY(ctx, hipMemcpyAsync(st.data(), b->bv.lm_state + d.lm0, (size_t)d.n_lm, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int l = 0; l < d.n_lm; ++l)  // packed order -> the caller's order; in the problem at create(), out of it now
        removed[b->P.lm_id[d.lm0 + l]] = (b->P.lm_state[d.lm0 + l] != 0 && st[l] == 0) ? 1 : 0;
    return LIMO_OK;
}

void limo_ba_batch_destroy(limo_ba_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    delete b;
}

int limo_ba_batch_kernel_stats(limo_ba_batch* b, int reset, double* linearize_ms, int64_t* linearize_launches,
                               double* total_ms) {
    if (!b) return LIMO_ERR_INVALID;
    int rc = b->collect_linearize_events();
    if (rc != LIMO_OK) return rc;
    if (linearize_ms) *linearize_ms = b->k_ms_acc[LIMO_KERNEL_LINEARIZE];
    if (linearize_launches) *linearize_launches = b->k_launches[LIMO_KERNEL_LINEARIZE];
    if (total_ms) *total_ms = b->total_ms_acc;
    if (reset) {
        for (int k = 0; k < 2; ++k) {
            b->k_ms_acc[k] = 0.0;
            b->k_launches[k] = 0;
        }
        b->total_ms_acc = 0.0;
    }
    return LIMO_OK;
}

int limo_ba_batch_kernel_time(limo_ba_batch* b, int kernel, double* ms, int64_t* launches) {
    if (!b || kernel < 0 || kernel > LIMO_KERNEL_SCHUR) return LIMO_ERR_INVALID;
    int rc = b->collect_linearize_events();
    if (rc != LIMO_OK) return rc;
    if (ms) *ms = b->k_ms_acc[kernel];
    if (launches) *launches = b->k_launches[kernel];
    return LIMO_OK;
}

int limo_comm_unique_id(unsigned char id[LIMO_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) <= LIMO_COMM_ID_BYTES, "ncclUniqueId does not fit");
    if (!id) return LIMO_ERR_INVALID;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return LIMO_ERR_RUNTIME;
    std::memset(id, 0, LIMO_COMM_ID_BYTES);
    std::memcpy(id, &u, sizeof(u));
    return LIMO_OK;
}

int limo_ctx_comm_init(limo_ctx* ctx, const unsigned char id[LIMO_COMM_ID_BYTES], int rank, int world) {
    if (!ctx || !id || world < 1 || rank < 0 || rank >= world) return LIMO_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;
    if (ctx->comm) {
        (void)ncclCommDestroy((ncclComm_t)ctx->comm);
        ctx->comm = nullptr;
    }
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    ncclResult_t r = ncclCommInitRank(&comm, world, u, rank);
    if (r != ncclSuccess) {
        ctx->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r);
        return LIMO_ERR_RUNTIME;
    }
    ctx->comm = comm;
    ctx->xfn = nullptr;
    ctx->comm_rank = rank;
    ctx->comm_world = world;
    return LIMO_OK;
}

int limo_ctx_comm_init_host(limo_ctx* ctx, limo_exchange_fn fn, void* user, int rank, int world) {
    if (!ctx || (fn && (world < 1 || rank < 0 || rank >= world))) return LIMO_ERR_INVALID;
    if (ctx->comm) {
        (void)ncclCommDestroy((ncclComm_t)ctx->comm);
        ctx->comm = nullptr;
    }
    ctx->xfn = fn;
    ctx->xuser = user;
    ctx->comm_rank = fn ? rank : 0;
    ctx->comm_world = fn ? world : 1;
    return LIMO_OK;
}

int limo_ba_solve_sharded(limo_ctx* ctx, limo_ba_window* window, const limo_ba_options* opts, int n_shards,
                          limo_ba_report* report) {
    if (!ctx || !window) return LIMO_ERR_INVALID;
    const bool ranks = ctx->has_transport();
    if (n_shards < 1 || (ranks && n_shards % ctx->comm_world != 0) || n_shards > 8 * (ranks ? ctx->comm_world : 1)) {
        ctx->err = "limo_ba_solve_sharded: n_shards must be a multiple of the communicator size, at most 8 shards per GPU";
        return LIMO_ERR_INVALID;
    }
    PackOptions po;
    po.shards = n_shards;
    limo_ba_batch* b = nullptr;
    ctx->last_log.clear();  // (no iteration log on this path: limo_ctx_last_iteration_log reports zero entries after it)
    ctx->last_log_n.clear();
    ctx->last_log_off.clear();
    int rc = batch_create_impl(ctx, 1, window, opts, po, &b, ranks);
    if (rc != LIMO_OK) return rc;
    rc = limo_ba_batch_solve(b, opts);
    limo_ba_report rep;
    if (rc == LIMO_OK) rc = limo_ba_batch_download(b, window, &rep);
    if (rc == LIMO_OK && report) *report = rep;
    ctx->exchange_stats[0] = b->n_exchanges;
    ctx->exchange_stats[1] = b->exchange_bytes;
    ctx->exchange_stats[2] = rc == LIMO_OK ? rep.iterations_total : 0;
    limo_ba_batch_destroy(b);
    return rc;
}

// The calls that take windows and give results back (limo_ba_solve, limo_ba_adjust_pose_only, limo_ba_adjust_pose_only_batch): create,
// solve, download, destroy over `n` windows.  KBA_HOST_TRACE=1 prints where the host time of the call goes.
static int solve_n(limo_ctx* ctx, int32_t n, limo_ba_window* windows, const limo_ba_options* opts, const PackOptions& po, limo_ba_report* reports,
                   const char* what) {
    using Clock = std::chrono::steady_clock;
    static const bool trace = std::getenv("KBA_HOST_TRACE") != nullptr;
    const auto t_a = Clock::now();
    limo_ba_batch* b = nullptr;
    int rc = batch_create_impl(ctx, n, windows, opts, po, &b);
    if (rc != LIMO_OK) return rc;
    const auto t0 = Clock::now();
    rc = limo_ba_batch_solve(b, nullptr);
    const auto t1 = Clock::now();
    if (rc == LIMO_OK) rc = limo_ba_batch_download(b, windows, reports);
    {   // the windows' iteration logs outlive the batch in the context's buffer (empty with the switch off)
        const int lrc = b->export_log();
        if (rc == LIMO_OK) rc = lrc;
    }
    const auto t2 = Clock::now();
    if (reports)
        for (int w = 0; w < n; ++w) reports[w].time_sec = std::chrono::duration<double>(t2 - t0).count();
    limo_ba_batch_destroy(b);
    if (trace) {
        auto us = [](Clock::time_point a, Clock::time_point c) { return std::chrono::duration<double, std::micro>(c - a).count(); };
        std::fprintf(stderr, "[kba] %s (%d windows): create %.0f us, solve %.0f us, download %.0f us, destroy %.0f us\n", what, (int)n, us(t_a, t0), us(t0, t1),
                     us(t1, t2), us(t2, Clock::now()));
    }
    return rc;
}

int64_t limo_ctx_coop_fallbacks(const limo_ctx* ctx) { return ctx ? (int64_t)ctx->coop_fallbacks : 0; }

int limo_ctx_exchange_stats(limo_ctx* ctx, int64_t* stats3) {
    if (!ctx || !stats3) return LIMO_ERR_INVALID;
    for (int i = 0; i < 3; ++i) stats3[i] = ctx->exchange_stats[i];
    return LIMO_OK;
}

int limo_ctx_last_solve_info(const limo_ctx* ctx, int64_t info[8]) {
    if (!ctx || !info) return LIMO_ERR_INVALID;
    for (int i = 0; i < 8; ++i) info[i] = ctx->last_solve_info[i];
    return LIMO_OK;
}

int limo_ctx_last_cam_lanes_info(const limo_ctx* ctx, int64_t info[9]) {
    if (!ctx || !info) return LIMO_ERR_INVALID;
    for (int i = 0; i < 9; ++i) info[i] = ctx->last_cam_lanes_info[i];
    return LIMO_OK;
}

int limo_ctx_last_schur_gp_info(const limo_ctx* ctx, int64_t info[4]) {
    if (!ctx || !info) return LIMO_ERR_INVALID;
    for (int i = 0; i < 4; ++i) info[i] = ctx->last_schur_gp_info[i];
    return LIMO_OK;
}

int limo_ctx_set_iteration_log(limo_ctx* ctx, int32_t on) {
    if (!ctx) return LIMO_ERR_INVALID;
    ctx->iteration_log = on != 0;
    return LIMO_OK;
}

// the argument checks the two readers share; null: the arguments are fine
static const char* iteration_log_args(int32_t window, int32_t n_win, int32_t cap, const limo_ba_iteration* out, const int32_t* n) {
    if (!n) return "n is NULL";
    if (cap < 0) return "cap < 0";
    if (cap > 0 && !out) return "out is NULL with cap > 0";
    if (window < 0 || (n_win >= 0 && window >= n_win)) return "window out of range";
    return nullptr;
}

int limo_ba_batch_iteration_log(limo_ba_batch* b, int32_t window, int32_t cap, limo_ba_iteration* out, int32_t* n) {
    if (!b) return LIMO_ERR_INVALID;
    limo_ctx* ctx = b->ctx;
    if (const char* bad = iteration_log_args(window, b->P.n_win, cap, out, n)) {
        ctx->err = std::string("limo_ba_batch_iteration_log: ") + bad;
        return LIMO_ERR_INVALID;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;
    return b->read_log(window, cap, out, n);
}

int limo_ctx_last_iteration_log(limo_ctx* ctx, int32_t window, int32_t cap, limo_ba_iteration* out, int32_t* n) {
    if (!ctx) return LIMO_ERR_INVALID;
    // (no log held - switch off, or limo_ba_solve_sharded: zero entries for any window)
    const int32_t n_win = ctx->last_log_n.empty() ? -1 : (int32_t)ctx->last_log_n.size();
    if (const char* bad = iteration_log_args(window, n_win, cap, out, n)) {
        ctx->err = std::string("limo_ctx_last_iteration_log: ") + bad;
        return LIMO_ERR_INVALID;
    }
    *n = 0;
    if (n_win < 0) return LIMO_OK;
    *n = ctx->last_log_n[window];
    const int m = std::min(*n, cap);
    if (m > 0) std::memcpy(out, ctx->last_log.data() + ctx->last_log_off[window], sizeof(limo_ba_iteration) * m);
    return LIMO_OK;
}

int limo_ba_solve(limo_ctx* ctx, limo_ba_window* window, const limo_ba_options* opts, limo_ba_report* report) {
    if (!ctx || !window) return LIMO_ERR_INVALID;
    return solve_n(ctx, 1, window, opts, PackOptions(), report, "limo_ba_solve");
}

int limo_ba_solve_fixed_landmarks(limo_ctx* ctx, limo_ba_window* window, const uint8_t* lm_fixed, const limo_ba_options* opts,
                                  limo_ba_report* report) {
    if (!ctx || !window) return LIMO_ERR_INVALID;
    PackOptions po;
    po.lm_fixed = lm_fixed ? &lm_fixed : nullptr;
    return solve_n(ctx, 1, window, opts, po, report, "limo_ba_solve_fixed_landmarks");
}

int limo_ba_batch_create_fixed_landmarks(limo_ctx* ctx, int32_t n_windows, const limo_ba_window* windows, const uint8_t* const* lm_fixed,
                                         limo_ba_batch** out) {
    // (do_trim from the default options here, refreshed by limo_ba_batch_solve(opts): as limo_ba_batch_create)
    PackOptions po;
    po.lm_fixed = lm_fixed;
    return batch_create_impl(ctx, n_windows, windows, nullptr, po, out);
}

int limo_ba_adjust_pose_only(limo_ctx* ctx, limo_ba_window* window, const limo_speed_prior* prior,
                             const limo_ba_options* opts, limo_ba_report* report) {
    if (!ctx || !window) return LIMO_ERR_INVALID;
    PackOptions po;
    po.pose_only = true;
    po.prior = prior;
    return solve_n(ctx, 1, window, opts, po, report, "limo_ba_adjust_pose_only");
}

int limo_ba_batch_create_pose_only(limo_ctx* ctx, int32_t n_windows, const limo_ba_window* windows, const limo_speed_prior* priors,
                                   limo_ba_batch** out) {
    // (do_trim from the default options here, refreshed by limo_ba_batch_solve(opts): as limo_ba_batch_create)
    PackOptions po;
    po.pose_only = true;
    po.per_window_prior = true;
    po.window_priors = priors;
    return batch_create_impl(ctx, n_windows, windows, nullptr, po, out);
}

int limo_ba_adjust_pose_only_batch(limo_ctx* ctx, int32_t n_windows, limo_ba_window* windows, const limo_speed_prior* priors,
                                   const limo_ba_options* opts, limo_ba_report* reports) {
    PackOptions po;
    po.pose_only = true;
    po.per_window_prior = true;
    po.window_priors = priors;
    return solve_n(ctx, n_windows, windows, opts, po, reports, "limo_ba_adjust_pose_only_batch");
}

int limo_ba_evaluate(limo_ctx* ctx, const limo_ba_window* window, const limo_ba_options* opts, int apply_loss,
                     double* cost, double* residuals, double* jac_pose, double* jac_lm, uint8_t* valid) {
    if (!ctx || !window) return LIMO_ERR_INVALID;
    PackOptions po;
    po.evaluate_only = true;
    limo_ba_batch* b = nullptr;
    int rc = batch_create_impl(ctx, 1, window, opts, po, &b);
    if (rc != LIMO_OK) return rc;
    const PackedBatch& P = b->P;
    const int M = P.TO, NB = std::max(1, P.n_echunk);
    double* d_cost = nullptr;
    uint8_t* d_valid = nullptr;
    rc = b->dmalloc((void**)&d_cost, sizeof(double) * NB);
    if (rc == LIMO_OK) rc = b->dmalloc((void**)&d_valid, (size_t)std::max(1, M) + 2);
    if (rc == LIMO_OK && P.n_echunk) {
        b->launch_evaluate(apply_loss, d_cost, d_valid);
        if (hipGetLastError() != hipSuccess) rc = LIMO_ERR_RUNTIME;
    }
    // device layout (kba_layout.hpp): rows u, v as planes over the observations, the depth row as compact planes over the depth observations
    const size_t SO = (size_t)P.SO, SD = (size_t)P.SD;
    std::vector<double> hr(2 * SO + SD), hjp(12 * SO + 6 * SD), hjl(6 * SO + 3 * SD), hc(NB, 0.0);
    std::vector<uint8_t> hv(std::max(1, M));
    if (rc == LIMO_OK) {
        hipError_t e = hipMemcpyAsync(hr.data(), b->bv.obs_r, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hjp.data(), b->bv.obs_Jp, sizeof(double) * hjp.size(), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hjl.data(), b->bv.obs_Jl, sizeof(double) * hjl.size(), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && P.n_echunk) e = hipMemcpyAsync(hc.data(), d_cost, sizeof(double) * NB, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hv.data(), d_valid, std::max(1, M), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ctx->err = std::string("evaluate: ") + hipGetErrorString(e);
            rc = LIMO_ERR_RUNTIME;
        }
    }
    if (rc == LIMO_OK) {
        double total = 0.0;
        for (int q = 0; q < P.n_echunk; ++q) total += hc[q];
        for (int o = 0; o < M; ++o) {
            const int src = P.obs_src[o];
            if (src < 0) continue;  // (padding of a view's segment)
            const bool dep = P.obs_rank[o] >= 0;
            const size_t rank = dep ? (size_t)P.obs_rank[o] : 0;
            if (valid) valid[src] = hv[o];
            if (residuals) {
                residuals[3 * (size_t)src + 0] = hr[o];
                residuals[3 * (size_t)src + 1] = hr[SO + o];
                residuals[3 * (size_t)src + 2] = dep ? hr[2 * SO + rank] : 0.0;
            }
            if (jac_pose)
                for (int i = 0; i < 6; ++i) {
                    jac_pose[18 * (size_t)src + i] = hjp[(size_t)i * SO + o];
                    jac_pose[18 * (size_t)src + 6 + i] = hjp[(size_t)(6 + i) * SO + o];
                    jac_pose[18 * (size_t)src + 12 + i] = dep ? hjp[12 * SO + (size_t)i * SD + rank] : 0.0;
                }
            if (jac_lm)
                for (int i = 0; i < 3; ++i) {
                    jac_lm[9 * (size_t)src + i] = hjl[(size_t)i * SO + o];
                    jac_lm[9 * (size_t)src + 3 + i] = hjl[(size_t)(3 + i) * SO + o];
                    jac_lm[9 * (size_t)src + 6 + i] = dep ? hjl[6 * SO + (size_t)i * SD + rank] : 0.0;
                }
        }
        if (cost) *cost = total;
    }
    limo_ba_batch_destroy(b);
    return rc;
}

int limo_ba_evaluate_rows(limo_ctx* ctx, const limo_ba_window* window, const limo_speed_prior* prior, int pose_only,
                          const limo_ba_options* opts, int32_t cap, limo_ba_row* rows, int32_t* n_rows) {
    if (!ctx || !window || !n_rows || cap < 0 || (cap > 0 && !rows)) return LIMO_ERR_INVALID;
    PackOptions po;
    po.pose_only = pose_only != 0;
    po.prior = pose_only ? prior : nullptr;
    limo_ba_batch* b = nullptr;
    int rc = batch_create_impl(ctx, 1, window, opts, po, &b);  // the SOLVE problem: ground-plane wiring, regularisers, constness
    if (rc != LIMO_OK) return rc;
    const PackedBatch& P = b->P;
    const WinDesc& wd = P.win[0];
    const int n_reg = reg_row_count(wd), n_gp = wd.n_gp;
    RegRow* d_rows = nullptr;
    int32_t* d_fixed = nullptr;
    rc = b->dmalloc((void**)&d_rows, sizeof(RegRow) * std::max(1, n_reg));
    if (rc == LIMO_OK) rc = b->dmalloc((void**)&d_fixed, sizeof(int32_t) * std::max(1, n_reg));
    std::vector<RegRow> hrows(std::max(1, n_reg));
    std::vector<int32_t> hfixed(std::max(1, n_reg));
    std::vector<double> gr(std::max<int64_t>(1, P.SG)), gF((size_t)std::max<int64_t>(1, P.SG) * 10), gE((size_t)std::max<int64_t>(1, P.SG) * 3), gcost(std::max(1, P.TG));
    if (rc == LIMO_OK) {
        hipLaunchKernelGGL(k_eval_rows, dim3(1), dim3(kBlock), 0, ctx->stream, b->bv, 0, d_rows, d_fixed);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && n_reg) e = hipMemcpyAsync(hrows.data(), d_rows, sizeof(RegRow) * n_reg, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && n_reg) e = hipMemcpyAsync(hfixed.data(), d_fixed, sizeof(int32_t) * n_reg, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && n_gp) e = hipMemcpyAsync(gr.data(), b->bv.gp_r, sizeof(double) * P.SG, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && n_gp) e = hipMemcpyAsync(gF.data(), b->bv.gp_F, sizeof(double) * P.SG * 10, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && n_gp) e = hipMemcpyAsync(gE.data(), b->bv.gp_E, sizeof(double) * P.SG * 3, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && n_gp) e = hipMemcpyAsync(gcost.data(), b->bv.gp_cost, sizeof(double) * P.TG, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ctx->err = std::string("evaluate_rows: ") + hipGetErrorString(e);
            rc = LIMO_ERR_RUNTIME;
        }
    }
    if (rc == LIMO_OK) *n_rows = rows_from_linearisation(P, 0, gr.data(), gF.data(), gE.data(), gcost.data(), hrows.data(), hfixed.data(), cap, rows);
    limo_ba_batch_destroy(b);
    return rc;
}

int limo_ba_evaluate_batch_time(limo_ctx* ctx, int32_t n, const limo_ba_window* windows, const limo_ba_options* opts, int32_t reps,
                                double* device_ms) {
    if (!ctx || !windows || n <= 0 || reps <= 0 || !device_ms) return LIMO_ERR_INVALID;
    PackOptions po;
    po.evaluate_only = true;
    limo_ba_batch* b = nullptr;
    int rc = batch_create_impl(ctx, n, windows, opts, po, &b);
    if (rc != LIMO_OK) return rc;
    const int M = b->P.TO;
    double* d_cost = nullptr;
    uint8_t* d_valid = nullptr;
    rc = b->dmalloc((void**)&d_cost, sizeof(double) * std::max(1, b->P.n_echunk));
    if (rc == LIMO_OK) rc = b->dmalloc((void**)&d_valid, (size_t)std::max(1, M) + 2);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (rc == LIMO_OK && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = LIMO_ERR_RUNTIME;
    if (rc == LIMO_OK && b->P.n_echunk) {
        hipStream_t s = ctx->stream;
        // (both launches of an evaluation are inside the timed region)
        b->launch_evaluate(1, d_cost, d_valid);  // warm-up
        (void)hipEventRecord(e0, s);
        for (int r = 0; r < reps; ++r) b->launch_evaluate(1, d_cost, d_valid);
        (void)hipEventRecord(e1, s);
        float ms = 0.f;
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
            ctx->err = "limo_ba_evaluate_batch_time: launch failed";
            rc = LIMO_ERR_RUNTIME;
        }
        *device_ms = ms / reps;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    limo_ba_batch_destroy(b);
    return rc;
}

}  // extern "C"
