// limo_ctx.hpp — the context object behind `limo_ctx*` (one per thread / GPU / stream), shared by the translation
// units that implement the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "kba_pack.hpp"

// Grow-only pinned host buffer: ensure() keeps what it has when that holds `bytes`, else it frees it and allocates
// max(bytes, min_bytes), at most max_bytes.  A failed allocation leaves the buffer empty.
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes, size_t min_bytes = 0, size_t max_bytes = ~size_t(0)) {
        if (cap >= bytes) return hipSuccess;
        release();
        const size_t want = std::min(max_bytes, std::max(bytes, min_bytes));
        const hipError_t e = hipHostMalloc(&p, want);
        if (e == hipSuccess)
            cap = want;
        else
            p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct limo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own = nullptr;
    std::string err;
    void* depth_ws = nullptr;               // workspace of limo_depth_estimate (depth.hip), grown on demand
    void (*depth_ws_free)(void*) = nullptr;
    void* comm = nullptr;                   // ncclComm_t of a landmark-sharded solve (limo_ctx_comm_init), else null
    int comm_rank = 0, comm_world = 1;
    // ... or a transport of the caller's (limo_ctx_comm_init_host): the exchange steps are staged through pinned host memory and
    // handed to this callback - how two processes that share ONE GPU (RCCL refuses a device twice in a communicator) or a host-side
    // fabric run the landmark-sharded solve with world > 1
    void (*xfn)(const double* send, double* recv, long long count, int kind, void* user) = nullptr;
    void* xuser = nullptr;
    PinnedBuf xhost;  // pinned staging: [1 + world][count] doubles
    bool has_transport() const { return comm != nullptr || xfn != nullptr; }
    long long exchange_stats[3] = {0, 0, 0};  // last landmark-sharded solve: exchange steps, bytes per rank, LM iterations
    long long coop_fallbacks = 0;           // one-launch solves whose barrier timed out and that were redone as a launch sequence
    int coop_strikes = 0;                   // ... in a row: after three the context stops taking the one-launch path (something shares the GPU)
    int coop_benched = 0;                   // solves kept off it since; the kCoopRetryAfter-th tries again (kba_batch_plan.hpp:choose_solve_path)
    long long last_solve_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // limo_ctx_last_solve_info: which path the last limo_ba_batch_solve took
    long long last_schur_gp_info[4] = {0, 0, 0, 0};           // limo_ctx_last_schur_gp_info: ... and which ground-plane Schur waves it ran
    long long last_cam_lanes_info[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // limo_ctx_last_cam_lanes_info: ... and which form its camera launches took
    // iteration log (limo_ctx_set_iteration_log): the switch limo_ba_batch_solve reads, and the logs of the windows of the last call
    // that made and destroyed its own batch (limo_ctx_last_iteration_log): window w has last_log_n[w] entries from last_log_off[w]
    bool iteration_log = false;
    std::vector<limo_ba_iteration> last_log;
    std::vector<int32_t> last_log_n;
    std::vector<size_t> last_log_off;
    // pose covariance (limo_ctx_set_pose_covariance): the switch every solve reads, and the matrices of the windows of the last call
    // that made and destroyed its own batch (limo_ctx_last_pose_covariance): window w has (6 n_kf)^2 doubles from last_cov_off[w].
    // last_cov_status empty: nothing held (switch off, limo_ba_solve_sharded) - LIMO_COV_NOT_COMPUTED for any window
    bool pose_covariance = false;
    std::vector<double> last_cov;
    std::vector<int32_t> last_cov_status;
    std::vector<size_t> last_cov_off;
    // limo_select_set_timing: HIP events around the kernels of limo_landmark_select[_batch]; the device time of the last call
    bool select_timing = false;
    double select_last_ms = 0.;
    // Device blocks released by finished batches, kept for the next one (size class = power of two): a single-window
    // call (limo_ba_solve, limo_ba_adjust_pose_only) would otherwise spend more time in hipMalloc / hipFree than in
    // its kernels.  At most kPoolPerClass blocks per class are kept; everything is freed with the context.
    static constexpr int kPoolPerClass = 4;
    static constexpr size_t kPoolMaxBlock = 32u << 20;  // larger blocks (big batches) go straight to hipMalloc / hipFree
    std::map<size_t, std::vector<void*>> pool, host_pool;  // device blocks / pinned host blocks
    PinnedBuf staging;                      // pinned host staging buffer of small uploads
    // Pinned host arena the big arrays of ONE batch's packing are carved from (kba_pack.hpp:PackArena): grow-only up to kPackArenaMax,
    // lent to a batch at its creation when no other live batch holds it, recycled when that batch is destroyed.  A batch packed into
    // it touches no fresh pages and uploads by DMA straight from where the pack wrote (1024 C2 windows: create 21 -> ~14 ms).
    PinnedBuf pack_arena;
    size_t pack_arena_wanted = 0;           // what the last batch that did not fit would have needed
    bool pack_arena_busy = false;
    static constexpr size_t kPackArenaMax = size_t(1) << 30;
    PinnedBuf staging_big;                  // pinned host buffer the results of a LARGE batch come back through (<= kBigStageMax)
    static constexpr size_t kBigStageMax = 512u << 20;

    // Larger blocks (the arena of a 1024-window batch is ~1.5 GB) are kept too, in 64 MB classes, one per class and at most
    // kPoolLargeBytes altogether: hipMalloc / hipFree of blocks that size synchronise the DEVICE, so a caller that streams
    // batches through two contexts (pack + upload of batch k + 1 under the solve of batch k) would otherwise serialise on them.
    static constexpr size_t kLargeStep = 64u << 20;
    static constexpr size_t kPoolLargeBytes = size_t(16) << 30;
    size_t pooled_large = 0;
    static size_t size_class(size_t bytes) {
        if (bytes > kPoolMaxBlock) return (bytes + kLargeStep - 1) / kLargeStep * kLargeStep;
        size_t c = 256;
        while (c < bytes) c <<= 1;
        return c;
    }
    hipError_t pool_alloc(void** p, size_t bytes) {
        const size_t c = size_class(bytes);
        static const bool no_reuse = std::getenv("KBA_NO_POOL") != nullptr;  // debugging aid
        if (no_reuse) return hipMalloc(p, c);
        auto it = pool.find(c);
        if (it != pool.end() && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            if (bytes > kPoolMaxBlock) pooled_large -= c;
            return hipSuccess;
        }
        hipError_t e = hipMalloc(p, c);
        // Out of memory with idle blocks in the pool (a caller whose batches vary in size leaves one multi-GB block per 64 MB
        // class behind; several contexts may share the GPU): give the idle blocks back, largest first, and try again - the
        // pool may cost time, never an allocation that would have succeeded without it.
        while (e == hipErrorOutOfMemory && trim_largest()) {
            (void)hipGetLastError();
            e = hipMalloc(p, c);
        }
        return e;
    }
    // frees the largest idle device block of the pool; false when the pool holds none
    bool trim_largest() {
        for (auto it = pool.rbegin(); it != pool.rend(); ++it) {
            if (it->second.empty()) continue;
            (void)hipFree(it->second.back());
            it->second.pop_back();
            if (it->first > kPoolMaxBlock) pooled_large -= it->first;
            return true;
        }
        return false;
    }
    void pool_free(void* p, size_t bytes) {
        const size_t c = size_class(bytes);
        auto& v = pool[c];
        static const bool no_reuse = std::getenv("KBA_NO_POOL") != nullptr;
        const bool large = bytes > kPoolMaxBlock;
        if (!no_reuse && (large ? (v.empty() && pooled_large + c <= kPoolLargeBytes) : (int)v.size() < kPoolPerClass)) {
            v.push_back(p);
            if (large) pooled_large += c;
        } else {
            (void)hipFree(p);
        }
    }
    hipError_t host_alloc(void** p, size_t bytes) {
        const size_t c = size_class(bytes);
        auto it = host_pool.find(c);
        if (it != host_pool.end() && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            return hipSuccess;
        }
        return hipHostMalloc(p, c);
    }
    void host_free(void* p, size_t bytes) {
        auto& v = host_pool[size_class(bytes)];
        if ((int)v.size() < kPoolPerClass && bytes <= kPoolMaxBlock)
            v.push_back(p);
        else
            (void)hipHostFree(p);
    }
    void pool_release() {
        for (auto& kv : host_pool)
            for (void* p : kv.second) (void)hipHostFree(p);
        host_pool.clear();
        for (auto& kv : pool)
            for (void* p : kv.second) (void)hipFree(p);
        pool.clear();
        pooled_large = 0;
        xhost.release();
        staging.release();
        staging_big.release();
        if (pack_arena.p) kba::pack_arena_register(pack_arena.p, pack_arena.cap, false);
        pack_arena.release();
    }
};
