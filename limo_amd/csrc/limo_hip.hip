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
#include "kba_window_options.hpp"

using namespace kba;

#include "limo_ctx.hpp"

#include "limo_batch.hpp"

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
    if (po.shards > 1 && n != 1) {  // (what the lock-step solve relies on: a sharded batch never re-batches, LockStep::rebatch)
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
    ShardExchange& sh = b->shards;
    sh.n_shards = b->P.n_shards;
    sh.is_virtual = !shards_are_ranks;
    sh.rank = shards_are_ranks ? ctx->comm_rank : 0;
    if (sh.n_shards > 1) {  // shard s lives on rank s mod world (all of them here when there is no communicator)
        const int world = shards_are_ranks ? ctx->comm_world : 1, me = shards_are_ranks ? ctx->comm_rank : 0;
        for (int r = 0; r < sh.n_shards; ++r)
            if (r % world == me) sh.local.push_back(r);
        if (sh.local.size() > 8) {
            ctx->err = "at most 8 shards per GPU";
            return LIMO_ERR_INVALID;
        }
    } else {
        sh.local.push_back(0);
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

// The solve behind limo_ba_batch_solve (each == null: one set of options, no table in any view) and limo_ba_batch_solve_each
// (each: the windows' own options, which passed check_window_options and differ - opts is each[0]).
static int batch_solve_impl(limo_ba_batch* b, const limo_ba_options* opts, const limo_ba_options* each) {
    limo_ctx* ctx = b->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;
    if (opts && b->refresh_options(*opts) != LIMO_OK) return LIMO_ERR_RUNTIME;
    b->set_window_table(nullptr);
    if (each) {
        window_options_table(b->P.n_win, each, false, b->wopt_host);
        if (b->upload_window_table() != LIMO_OK) return LIMO_ERR_RUNTIME;
    }
    b->rc = LIMO_OK;
    // iteration log: every solve starts its windows' logs at zero entries (not offered for a landmark-sharded batch)
    if (b->log.bind(ctx->iteration_log && b->shards.n_shards == 1) != LIMO_OK) return LIMO_ERR_RUNTIME;
    if (b->timers.start_solve() != LIMO_OK) return LIMO_ERR_RUNTIME;
    // Which path (kba_batch_plan.hpp:choose_solve_path; the KBA_* switches are read per call: the tests switch paths).  All paths
    // give the same bits.
    b->run = {};
    b->run.sw = read_solve_switches();
    const SolveChoice ch = b->choose_path();
    b->run_path(ch);
    const int redo = b->one.recover();  // (a cooperative launch whose barrier timed out)
    if (redo < 0) return redo;
    if (redo) {
        b->launch_sequence(ch.fallback);
        b->pristine = false;
    }
    const int gathered = b->shards.gather_landmarks();
    if (gathered != LIMO_OK) return gathered;
    b->publish_run();
    // pose covariance: the pass behind the solve's last launch, after the record of the solve is taken (its launches are not the solve's)
    b->cov.computed = false;
    if (ctx->pose_covariance && b->rc == LIMO_OK && b->cov.run() != LIMO_OK) return LIMO_ERR_RUNTIME;
    if (b->timers.stop_solve() != LIMO_OK) return LIMO_ERR_RUNTIME;
    return b->rc;
}

int limo_ba_batch_solve(limo_ba_batch* b, const limo_ba_options* opts) {
    if (!b) return LIMO_ERR_INVALID;
    return batch_solve_impl(b, opts, nullptr);
}

int limo_ba_batch_solve_each(limo_ba_batch* b, int32_t n_opts, const limo_ba_options* opts) {
    if (!b) return LIMO_ERR_INVALID;
    limo_ctx* ctx = b->ctx;
    if (b->shards.n_shards > 1) {
        ctx->err = "limo_ba_batch_solve_each: not offered for a landmark-sharded batch";
        return LIMO_ERR_INVALID;
    }
    bool uniform = true;
    std::string why;
    if (check_window_options(b->P.n_win, n_opts, opts, &uniform, why) != LIMO_OK) {  // (nothing has been launched)
        ctx->err = "limo_ba_batch_solve_each: " + why;
        return LIMO_ERR_INVALID;
    }
    return batch_solve_impl(b, &opts[0], uniform ? nullptr : opts);
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
            r.time_sec = b->timers.last_solve_sec;
        }
    };
    pack_parallel_for(P.n_win, std::min(32u, (unsigned)(P.n_win / 32)), 8, one_window);
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
    KernelTimers& t = b->timers;
    int rc = t.collect();
    if (rc != LIMO_OK) return rc;
    if (linearize_ms) *linearize_ms = t.k_ms_acc[LIMO_KERNEL_LINEARIZE];
    if (linearize_launches) *linearize_launches = t.k_launches[LIMO_KERNEL_LINEARIZE];
    if (total_ms) *total_ms = t.total_ms_acc;
    if (reset) {
        for (int k = 0; k < 2; ++k) {
            t.k_ms_acc[k] = 0.0;
            t.k_launches[k] = 0;
        }
        t.total_ms_acc = 0.0;
    }
    return LIMO_OK;
}

int limo_ba_batch_kernel_time(limo_ba_batch* b, int kernel, double* ms, int64_t* launches) {
    if (!b || kernel < 0 || kernel > LIMO_KERNEL_SCHUR) return LIMO_ERR_INVALID;
    int rc = b->timers.collect();
    if (rc != LIMO_OK) return rc;
    if (ms) *ms = b->timers.k_ms_acc[kernel];
    if (launches) *launches = b->timers.k_launches[kernel];
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
    ctx->last_cov.clear();  // (nor a pose covariance: LIMO_COV_NOT_COMPUTED)
    ctx->last_cov_status.clear();
    ctx->last_cov_off.clear();
    int rc = batch_create_impl(ctx, 1, window, opts, po, &b, ranks);
    if (rc != LIMO_OK) return rc;
    b->cov.offered = false;  // (also with one shard: the call reports none, so it does not pay for the pass)
    rc = limo_ba_batch_solve(b, opts);
    limo_ba_report rep;
    if (rc == LIMO_OK) rc = limo_ba_batch_download(b, window, &rep);
    if (rc == LIMO_OK && report) *report = rep;
    ctx->exchange_stats[0] = b->shards.n_exchanges;
    ctx->exchange_stats[1] = b->shards.exchange_bytes;
    ctx->exchange_stats[2] = rc == LIMO_OK ? rep.iterations_total : 0;
    limo_ba_batch_destroy(b);
    return rc;
}

// The calls that take windows and give results back (limo_ba_solve, limo_ba_adjust_pose_only, limo_ba_adjust_pose_only_batch): create,
// solve, download, destroy over `n` windows.  KBA_HOST_TRACE=1 prints where the host time of the call goes.
static int solve_n(limo_ctx* ctx, int32_t n, limo_ba_window* windows, const limo_ba_options* opts, const PackOptions& po, limo_ba_report* reports,
                   const char* what, const limo_ba_options* each = nullptr) {
    using Clock = std::chrono::steady_clock;
    static const bool trace = std::getenv("KBA_HOST_TRACE") != nullptr;
    const auto t_a = Clock::now();
    limo_ba_batch* b = nullptr;
    int rc = batch_create_impl(ctx, n, windows, opts, po, &b);
    if (rc != LIMO_OK) return rc;
    const auto t0 = Clock::now();
    rc = each ? limo_ba_batch_solve_each(b, n, each) : limo_ba_batch_solve(b, nullptr);  // (each: the windows' own options; opts is each[0])
    if (rc != LIMO_OK && each) {
        limo_ba_batch_destroy(b);
        return rc;
    }
    const auto t1 = Clock::now();
    if (rc == LIMO_OK) rc = limo_ba_batch_download(b, windows, reports);
    {   // the windows' iteration logs outlive the batch in the context's buffer (empty with the switch off)
        const int lrc = b->log.export_to_ctx();
        if (rc == LIMO_OK) rc = lrc;
        const int crc = b->cov.export_to_ctx();  // (and their pose covariances)
        if (rc == LIMO_OK) rc = crc;
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
    return b->log.read(window, cap, out, n);
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

int limo_ctx_set_pose_covariance(limo_ctx* ctx, int32_t on) {
    if (!ctx) return LIMO_ERR_INVALID;
    ctx->pose_covariance = on != 0;
    return LIMO_OK;
}

// the argument checks the two readers share (n_win < 0: nothing held, any window >= 0 passes); null: the arguments are fine
static const char* pose_covariance_args(int32_t window, int32_t n_win, int64_t cap, const double* out, const int32_t* status) {
    if (!status) return "status is NULL";
    if (cap < 0) return "cap_doubles < 0";
    if (cap > 0 && !out) return "out is NULL with cap_doubles > 0";
    if (window < 0 || (n_win >= 0 && window >= n_win)) return "window out of range";
    return nullptr;
}

int limo_ba_batch_pose_covariance(limo_ba_batch* b, int32_t window, int64_t cap_doubles, double* out, int32_t* status) {
    if (!b) return LIMO_ERR_INVALID;
    limo_ctx* ctx = b->ctx;
    if (const char* bad = pose_covariance_args(window, b->P.n_win, cap_doubles, out, status)) {
        ctx->err = std::string("limo_ba_batch_pose_covariance: ") + bad;
        return LIMO_ERR_INVALID;
    }
    if (out && b->cov.computed && cap_doubles < b->cov.cov_off[window + 1] - b->cov.cov_off[window]) {
        ctx->err = "limo_ba_batch_pose_covariance: cap_doubles < (6 n_kf)^2";
        return LIMO_ERR_INVALID;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;
    return b->cov.read(window, cap_doubles, out, status);
}

int limo_ctx_last_pose_covariance(limo_ctx* ctx, int32_t window, int64_t cap_doubles, double* out, int32_t* status) {
    if (!ctx) return LIMO_ERR_INVALID;
    const int32_t n_win = ctx->last_cov_status.empty() ? -1 : (int32_t)ctx->last_cov_status.size();
    if (const char* bad = pose_covariance_args(window, n_win, cap_doubles, out, status)) {
        ctx->err = std::string("limo_ctx_last_pose_covariance: ") + bad;
        return LIMO_ERR_INVALID;
    }
    *status = LIMO_COV_NOT_COMPUTED;
    if (n_win < 0) return LIMO_OK;
    const size_t n = ctx->last_cov_off[window + 1] - ctx->last_cov_off[window];
    if (out && (size_t)cap_doubles < n) {
        ctx->err = "limo_ctx_last_pose_covariance: cap_doubles < (6 n_kf)^2";
        return LIMO_ERR_INVALID;
    }
    *status = ctx->last_cov_status[window];
    if (out && n) std::memcpy(out, ctx->last_cov.data() + ctx->last_cov_off[window], sizeof(double) * n);
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

int limo_ba_adjust_pose_only_batch_each(limo_ctx* ctx, int32_t n_windows, limo_ba_window* windows, const limo_speed_prior* priors,
                                        const limo_ba_options* opts, limo_ba_report* reports) {
    if (!ctx) return LIMO_ERR_INVALID;
    if (!windows || n_windows <= 0) {
        ctx->err = "limo_ba_adjust_pose_only_batch_each: no windows";
        return LIMO_ERR_INVALID;
    }
    bool uniform = true;
    std::string why;
    if (check_window_options(n_windows, n_windows, opts, &uniform, why) != LIMO_OK) {  // (before anything is packed or launched)
        ctx->err = "limo_ba_adjust_pose_only_batch_each: " + why;
        return LIMO_ERR_INVALID;
    }
    if (uniform) return limo_ba_adjust_pose_only_batch(ctx, n_windows, windows, priors, &opts[0], reports);
    PackOptions po;
    po.pose_only = true;
    po.per_window_prior = true;
    po.window_priors = priors;
    return solve_n(ctx, n_windows, windows, &opts[0], po, reports, "limo_ba_adjust_pose_only_batch_each", opts);
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
