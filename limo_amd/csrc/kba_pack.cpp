// kba_pack.cpp — see kba_pack.hpp.
#include "kba_pack.hpp"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <limits>
#include <mutex>
#include <numeric>
#include <thread>
#include <pthread.h>
#include <unistd.h>
#include <exception>

#include "kba_items.hpp"

namespace kba {

// ---- the arena of the big pack arrays (kba_pack.hpp:PackArena)
namespace {
thread_local PackArena* t_pack_arena = nullptr;
std::mutex g_arena_ranges_m;
std::vector<std::pair<const char*, size_t>> g_arena_ranges;
std::atomic<int> g_arena_range_count{0};  // (pack_arena_owns is on every deallocation path: no lock while no arena exists)
}  // namespace
void pack_arena_lend(PackArena* a) { t_pack_arena = a; }
void pack_arena_register(const void* base, size_t cap, bool add) {
    std::lock_guard<std::mutex> lk(g_arena_ranges_m);
    if (add) {
        g_arena_ranges.emplace_back(static_cast<const char*>(base), cap);
    } else {
        for (size_t i = 0; i < g_arena_ranges.size(); ++i)
            if (g_arena_ranges[i].first == base) {
                g_arena_ranges.erase(g_arena_ranges.begin() + i);
                break;
            }
    }
    g_arena_range_count.store((int)g_arena_ranges.size(), std::memory_order_release);
}
bool pack_arena_owns(const void* p) {
    if (g_arena_range_count.load(std::memory_order_acquire) == 0) return false;
    std::lock_guard<std::mutex> lk(g_arena_ranges_m);
    const char* q = static_cast<const char*>(p);
    for (const auto& r : g_arena_ranges)
        if (q >= r.first && q < r.first + r.second) return true;
    return false;
}
void* pack_arena_take(size_t bytes) {
    PackArena* a = t_pack_arena;
    if (!a) return nullptr;
    const size_t need = (bytes + 255) / 256 * 256;
    a->wanted += need;
    if (!a->base || a->used + need > a->cap) return nullptr;
    void* p = a->base + a->used;
    a->used += need;
    return p;
}

namespace {
inline int64_t pad64(int64_t n) {
    return (n + 63) / 64 * 64;
}

// Host threads of the pack, kept between calls: a 1024-window create runs three parallel passes, and spawning 64 threads for each of
// them cost more than the passes' own work on a busy 256-thread host.  One parallel region at a time (a second caller - another host
// thread packing for another context - finds the pool busy and spawns its own threads as before); the caller takes part in the work.
//   * The caller only waits for the workers that JOINED the region: a worker that wakes after the items have run out (a loaded host)
//     finds the region closed and goes back to sleep - nobody waits for threads the scheduler has not run yet.
//   * An exception thrown by f on a worker is caught there and rethrown by run() on the caller (the first one wins).
//   * The pool is never destroyed (its threads sleep on a condition variable until the process ends).  A forked child gets a FRESH pool
//     object (pthread_atfork): the parent's threads do not exist there and its mutexes may have been held at the fork.
class PackPool {
public:
    // runs f(0 .. n - 1) on up to nt threads (the caller included); false = busy, nothing done
    bool run(unsigned nt, int n, const std::function<void(int)>& f) {
        std::unique_lock<std::mutex> region(region_, std::try_to_lock);
        if (!region.owns_lock()) return false;
        {
            std::lock_guard<std::mutex> lk(m_);
            while (threads_.size() + 1 < nt) {
                threads_.emplace_back([this] { worker(); });
                threads_.back().detach();
            }
            fn_ = &f;
            n_ = n;
            next_.store(0);
            want_ = std::min<size_t>(threads_.size(), nt > 0 ? nt - 1 : 0);
            joined_ = 0;
            open_ = true;
            error_ = nullptr;
            ++gen_;
        }
        cv_.notify_all();
        std::exception_ptr mine;
        try {
            for (int i = next_.fetch_add(1); i < n; i = next_.fetch_add(1)) f(i);
        } catch (...) {
            mine = std::current_exception();
            next_.store(n);  // (the workers stop taking items)
        }
        std::unique_lock<std::mutex> lk(m_);
        open_ = false;  // late wakers skip this region
        done_.wait(lk, [this] { return joined_ == 0; });
        fn_ = nullptr;
        std::exception_ptr e = mine ? mine : error_;
        error_ = nullptr;
        lk.unlock();
        if (e) std::rethrow_exception(e);
        return true;
    }

private:
    void worker() {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)>* f = nullptr;
            int n = 0;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (!open_ || want_ == 0) continue;  // closed already, or enough workers: not this region
                --want_;
                ++joined_;
                f = fn_;
                n = n_;
            }
            std::exception_ptr err;
            try {
                for (int i = next_.fetch_add(1); i < n; i = next_.fetch_add(1)) (*f)(i);
            } catch (...) {
                err = std::current_exception();
                next_.store(n);
            }
            {
                std::lock_guard<std::mutex> lk(m_);
                if (err && !error_) error_ = err;
                if (--joined_ == 0) done_.notify_one();
            }
        }
    }
    std::mutex region_, m_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> threads_;
    const std::function<void(int)>* fn_ = nullptr;
    std::atomic<int> next_{0};
    int n_ = 0, joined_ = 0;
    bool open_ = false;
    size_t want_ = 0;
    uint64_t gen_ = 0;
    std::exception_ptr error_;
};
std::atomic<PackPool*> g_pack_pool{nullptr};
void pack_pool_after_fork() { g_pack_pool.store(nullptr); }  // (the parent's object is abandoned in the child: its threads are not there)
PackPool& pack_pool() {
    PackPool* p = g_pack_pool.load(std::memory_order_acquire);
    if (!p) {
        static std::mutex make;
        static bool hooked = false;
        // (in a forked child `make` may have been copied in the locked state only if the fork raced the very first call; a process that
        // forks while it is creating its first batch is outside what this pool supports)
        std::lock_guard<std::mutex> lk(make);
        p = g_pack_pool.load(std::memory_order_acquire);
        if (!p) {
            p = new PackPool();  // (leaked on purpose: see the class comment)
            if (!hooked) {
                pthread_atfork(nullptr, nullptr, pack_pool_after_fork);
                hooked = true;
            }
            g_pack_pool.store(p, std::memory_order_release);
        }
    }
    return *p;
}
}  // namespace

SolveConsts make_consts(const limo_ba_options& o) {
    SolveConsts c;
    std::memset(&c, 0, sizeof(c));
    c.a_rep = o.reprojection_thres;
    c.a_dep = o.depth_thres;
    c.inv_a_rep2 = 1.0 / (c.a_rep * c.a_rep);
    c.inv_a_dep2 = 1.0 / (c.a_dep * c.a_dep);
    c.function_tolerance = o.function_tolerance;
    c.gradient_tolerance = o.gradient_tolerance;
    c.parameter_tolerance = o.parameter_tolerance;
    c.initial_radius = o.initial_trust_region_radius;
    c.max_radius = o.max_trust_region_radius;
    c.min_radius = o.min_trust_region_radius;
    c.min_lm_diagonal = o.min_lm_diagonal;
    c.max_lm_diagonal = o.max_lm_diagonal;
    c.min_relative_decrease = o.min_relative_decrease;
    c.max_invalid = o.max_num_consecutive_invalid_steps;
    c.jacobi_scaling = o.jacobi_scaling;
    c.depth_quantile = o.depth_quantile;
    c.reprojection_quantile = o.reprojection_quantile;
    c.min_groups = o.minimum_number_residual_groups;
    c.schur_span = 1;
    c.schur_span_gp = 1;
    c.num_trim_rounds = o.num_trim_rounds;
    c.trim_iters = o.trim_solver_iterations;
    c.max_iters = o.max_num_iterations;
    return c;
}

void pack_parallel_for(int n, unsigned max_threads, int grain, const std::function<void(int)>& f) {
    unsigned nt = std::min(std::thread::hardware_concurrency(), max_threads);
    if (const char* e = std::getenv("KBA_PACK_THREADS")) nt = (unsigned)std::max(1, std::atoi(e));
    if (nt <= 1) {
        for (int i = 0; i < n; ++i) f(i);
        return;
    }
    const int n_chunks = (n + grain - 1) / grain;
    const std::function<void(int)> chunk = [&](int c) {
        for (int i = c * grain; i < std::min(n, (c + 1) * grain); ++i) f(i);
    };
    if (pack_pool().run(nt, n_chunks, chunk)) return;
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&] {
            for (int c = next.fetch_add(1); c < n_chunks; c = next.fetch_add(1)) chunk(c);
        });
    for (auto& th : pool) th.join();
}

// ==================================================================================================================
// The problem's rules (kba_pack.hpp:WindowProblem).  Reference lines are bundle_adjuster_keyframes.cpp unless named.
// ==================================================================================================================
WindowProblem build_window_problem(const limo_ba_window& W, const limo_ba_options& opts, const PackOptions& po, int w) {
    WindowProblem pr;
    auto fail = [&](int code, const char* msg) {
        pr.rc = code;
        pr.err = msg;
        return pr;
    };
    // ---- validation
    if (W.n_kf < 0 || W.n_lm < 0 || W.n_obs < 0 || W.n_cam < 0) return fail(LIMO_ERR_INVALID, "negative size");
    // The reference's NotEnoughKeyframesException counts ALL pushed keyframes (keyframes_.size() < 3, :630) - that check lives in
    // the C++ shim.  The window only holds the ACTIVE ones, and the reference solves happily with two
    // (deactivateKeyframes(min_conn, 3, max) can leave exactly the two newest, mono_lidar.cpp:249) or one of them: the scale /
    // ground-plane regularisers simply need > 1 (:771, :891).  Only an empty window has nothing to solve.
    const bool solve = !po.pose_only && !po.evaluate_only;  // the full problem: ground plane, regularisers, constness
    if (solve && W.n_kf < 1) return fail(LIMO_ERR_NOT_ENOUGH_KF, "window without active keyframes");
    if (po.pose_only && W.n_kf != 1) return fail(LIMO_ERR_INVALID, "pose-only window must hold exactly one keyframe");
    if (W.n_kf > kMaxKf) return fail(LIMO_ERR_INVALID, "window has more keyframes than kMaxKf (20)");
    if ((W.n_kf && (!W.kf_pose || !W.kf_plane_dir || !W.kf_plane_dist || !W.kf_fixation)) ||
        (W.n_lm && (!W.lm_pos || !W.lm_weight || !W.lm_is_ground)) || (W.n_cam && !W.cam) ||
        (W.n_obs && (!W.obs_kf || !W.obs_lm || !W.obs_cam || !W.obs_u || !W.obs_v || !W.obs_d)))
        return fail(LIMO_ERR_INVALID, "null pointer in window");
    // ---- the residual blocks of the observations (:584-620): one reprojection block each, a depth block where d > 0
    std::vector<int> vid((size_t)W.n_kf * std::max(1, W.n_cam), -1);
    std::vector<int> lm_nobs(W.n_lm, 0), kf_obs(W.n_kf, 0);
    for (int i = 0; i < W.n_obs; ++i) {
        const int k = W.obs_kf[i], l = W.obs_lm[i], c = W.obs_cam[i];
        if (k < 0 || k >= W.n_kf || l < 0 || l >= W.n_lm || c < 0 || c >= W.n_cam)
            return fail(LIMO_ERR_INVALID, "observation index out of range");
        vid[(size_t)k * W.n_cam + c] = 0;
        lm_nobs[l]++;
        kf_obs[k]++;
        if (W.obs_d[i] > 0.0f) pr.n_depth++;
    }
    pr.n_repr = W.n_obs;
    // ---- constant landmarks (PackOptions::lm_fixed; deactivateLandmarks, :262-269): in the problem with every residual block they
    //      have, as constant parameter blocks
    pr.lm_const.assign(W.n_lm, 0);
    if (const uint8_t* fixed_in = (po.lm_fixed && solve) ? po.lm_fixed[w] : nullptr)
        for (int l = 0; l < W.n_lm; ++l) pr.n_const += pr.lm_const[l] = fixed_in[l] != 0;
    // ---- views.  Order: by keyframe, then camera.  A window with constant landmarks (a flag set) takes the views of ALL its
    //      LIMO_FIX_POSE keyframes first, wherever they stand in the window (each group by keyframe, then camera): they are the views
    //      without a free pose block, WinDesc::n_view_fixed0 then counts every one of them, and the fixed-cost rule for (pose-fixed
    //      keyframe, constant landmark) blocks holds for any kf_fixation pattern.  Windows without a flag set keep the plain order
    //      (their bits depend on it).
    const bool fixed_first = pr.n_const > 0;
    int nv = 0;
    for (int pass = fixed_first ? 0 : 1; pass < 2; ++pass)
        for (int k = 0; k < W.n_kf; ++k) {
            if (fixed_first && (W.kf_fixation[k] == LIMO_FIX_POSE) != (pass == 0)) continue;
            for (int c = 0; c < W.n_cam; ++c)
                if (vid[(size_t)k * W.n_cam + c] == 0) {
                    vid[(size_t)k * W.n_cam + c] = nv++;
                    pr.views.push_back({k, c});
                }
        }
    if (nv > kMaxViews) return fail(LIMO_ERR_INVALID, "window has more than kMaxViews (64) (keyframe, camera) views with observations");
    pr.obs_view.resize(W.n_obs);
    for (int i = 0; i < W.n_obs; ++i) pr.obs_view[i] = vid[(size_t)W.obs_kf[i] * W.n_cam + W.obs_cam[i]];
    // ---- ground-plane residuals, addGroundPlaneResiduals(10.), :517-562: a ground landmark hangs on the nearest keyframe that has a
    //      plane (kf_plane_dist >= -10), if that is closer than 25 m, with a weight that falls linearly to 0 there
    std::vector<uint8_t> has_gp(W.n_lm, 0);
    if (solve) {
        const double weight = 10.;
        double Rk[kMaxKf][9];  // (one rotation matrix per keyframe, not per (landmark, keyframe) pair)
        for (int k = 0; k < W.n_kf; ++k) quat_R(W.kf_pose + 7 * k, Rk[k]);
        for (int l = 0; l < W.n_lm; ++l) {
            if (!W.lm_is_ground[l]) continue;
            double min_dist = std::numeric_limits<double>::max();
            int kf_id = -1;
            for (int k = 0; k < W.n_kf; ++k) {
                if (W.kf_plane_dist[k] < -10.) continue;
                const double* R = Rk[k];
                double y[3];
                mat3_vec(R, W.lm_pos + 3 * l, y);
                y[0] += W.kf_pose[7 * k + 4];
                y[1] += W.kf_pose[7 * k + 5];
                y[2] += W.kf_pose[7 * k + 6];
                const double dist = std::sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
                if (dist < min_dist) {
                    min_dist = dist;
                    kf_id = k;
                }
            }
            if (kf_id < 0) continue;
            const double max_valid_dist = 25.;
            if (min_dist < max_valid_dist) {
                pr.gp.push_back({kf_id, l, weight * (1. - min_dist / max_valid_dist)});
                has_gp[l] = 1;
            }
        }
    }
    const int n_gp = (int)pr.gp.size();
    // ---- landmark states: in the problem with an observation (constant in a pose-only problem: adjustPoseOnly, :835-853) or with
    //      a ground-plane row alone; a flagged landmark that is in the problem is a constant block
    pr.lm_state.resize(W.n_lm);
    for (int l = 0; l < W.n_lm; ++l) {
        uint8_t s = lm_nobs[l] > 0 ? (po.pose_only ? 2 : 1) : 0;
        if (has_gp[l] && s == 0) s = 1;  // constrained by its gp block only
        if (pr.lm_const[l] && s == 1) s = 2;
        pr.lm_state[l] = s;
    }
    // ---- which camera-side parameter blocks exist / are free
    auto set_block = [&](std::array<uint8_t, kMaxKf * kCamSlots>& m, int k, int s0, int cnt) {
        for (int i = 0; i < cnt; ++i) m[k * kCamSlots + s0 + i] = 1;
    };
    if (po.evaluate_only) {
        for (int k = 0; k < W.n_kf; ++k) {
            set_block(pr.present, k, 0, 6);
            set_block(pr.free, k, 0, 6);
        }
    } else if (po.pose_only) {
        set_block(pr.present, 0, 0, 6);
        set_block(pr.free, 0, 0, 6);  // the new keyframe is not in active_keyframe_ids_, so never constant
        // the speed prior: the window's own in a batch of adjustPoseOnly problems, the call's otherwise
        const limo_speed_prior* prior = po.per_window_prior ? (po.window_priors ? po.window_priors + w : nullptr) : po.prior;
        if (prior && prior->speed_weight > 0.0) {
            pr.speed_w = prior->speed_weight;
            pr.speed_dt = prior->dt_cur;
            for (int i = 0; i < 3; ++i) pr.speed_vel[i] = prior->vel_prev[i];
            quat_R(prior->pose_before, pr.speed_Rb);
            for (int i = 0; i < 3; ++i) pr.speed_tb[i] = prior->pose_before[4 + i];
        }
    } else {
        // scale regularisation, :704-716 / :890-904
        const int n_depth = pr.n_depth;
        double scale_w = -1.0;
        if (n_depth > 10 || n_gp > 10) {
            if (n_gp < 30) scale_w = 1000. / (static_cast<double>(n_depth + static_cast<double>(n_gp)));
        } else {
            scale_w = 1000.;
        }
        if (scale_w > 0.0 && W.n_kf > 1) {
            pr.has_scale_reg = true;
            pr.scale_w = scale_w;
            double dd[3];
            rel_translation(W.kf_pose + 7, W.kf_pose, dd, nullptr, nullptr, false);
            pr.scale_s0 = std::sqrt(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]);
        }
        pr.has_gp_reg = n_gp > 0 && W.n_kf > 1;  // :717-719, :771
        std::vector<int> kf_gp(W.n_kf, 0);
        for (const WindowProblem::GpRow& g : pr.gp) kf_gp[g.kf]++;
        for (int k = 0; k < W.n_kf; ++k) {
            const bool pose_in = kf_obs[k] > 0 || kf_gp[k] > 0 || pr.has_gp_reg || (pr.has_scale_reg && k < 2);
            const bool plane_in = kf_gp[k] > 0 || pr.has_gp_reg;
            if (pose_in) set_block(pr.present, k, 0, 6);
            if (plane_in) set_block(pr.present, k, 6, 4);
            const bool fixed = W.kf_fixation[k] == LIMO_FIX_POSE;  // deactivatePoseParameters, :198-219
            if (pose_in && !fixed) set_block(pr.free, k, 0, 6);
            if (plane_in && !fixed) set_block(pr.free, k, 6, 3);
            if (plane_in && !fixed && !(n_depth < 10)) set_block(pr.free, k, 9, 1);  // :722-728
        }
    }
    pr.do_trim = W.n_lm > opts.min_landmarks_for_trimming;  // :741 / :865
    return pr;
}

// ==================================================================================================================
// The batch layout: where the blocks of every window's problem stand in the arrays of kba_layout.hpp.  Windows are
// independent: every window writes its own ranges of the fixed-size arrays and collects its variable-size lists
// (WinLists) with LOCAL indices; the merge concatenates them.
// ==================================================================================================================
namespace {

// The variable-size lists of a batch, by kind.  The columns of a kind have one entry per item; the table names every column
// once, for the sizes, the bases and the copies of the merge (merge_lists) alike.
enum ListKind { kObsBlocks, kLmBlocks, kSchurBlocks, kGpRows, kListKinds };
struct WinLists {
    std::vector<int32_t> blk_view, blk_obs0, blk_n, blk_owner;    // observation blocks (one view each)
    std::vector<int32_t> lblk_win, lblk_lm0, lblk_n, lblk_owner;  // landmark workgroups
    std::vector<int32_t> sblk_win, sblk_lm0, sblk_n, sblk_owner;  // Schur blocks
    std::vector<int32_t> gp_lm, gp_kf, gp_owner;                  // ground-plane rows
    std::vector<double> gp_w;
    std::string err;  // rc != LIMO_OK: why the window cannot be laid out
    int rc = LIMO_OK;
};
template <typename T>
struct ListColumn {
    ListKind kind;
    std::vector<T> WinLists::*local;
    std::vector<T> PackedBatch::*global;
};
const ListColumn<int32_t> kIntColumns[] = {
    {kObsBlocks, &WinLists::blk_view, &PackedBatch::blk_view},   {kObsBlocks, &WinLists::blk_obs0, &PackedBatch::blk_obs0},
    {kObsBlocks, &WinLists::blk_n, &PackedBatch::blk_n},         {kObsBlocks, &WinLists::blk_owner, &PackedBatch::blk_owner},
    {kLmBlocks, &WinLists::lblk_win, &PackedBatch::lblk_win},    {kLmBlocks, &WinLists::lblk_lm0, &PackedBatch::lblk_lm0},
    {kLmBlocks, &WinLists::lblk_n, &PackedBatch::lblk_n},        {kLmBlocks, &WinLists::lblk_owner, &PackedBatch::lblk_owner},
    {kSchurBlocks, &WinLists::sblk_win, &PackedBatch::sblk_win}, {kSchurBlocks, &WinLists::sblk_lm0, &PackedBatch::sblk_lm0},
    {kSchurBlocks, &WinLists::sblk_n, &PackedBatch::sblk_n},     {kSchurBlocks, &WinLists::sblk_owner, &PackedBatch::sblk_owner},
    {kGpRows, &WinLists::gp_lm, &PackedBatch::gp_lm},            {kGpRows, &WinLists::gp_kf, &PackedBatch::gp_kf},
    {kGpRows, &WinLists::gp_owner, &PackedBatch::gp_owner},
};
const ListColumn<double> kDoubleColumns[] = {{kGpRows, &WinLists::gp_w, &PackedBatch::gp_w}};
int list_count(const WinLists& L, ListKind kind) {  // (the length of the kind's first column)
    for (const ListColumn<int32_t>& c : kIntColumns)
        if (c.kind == kind) return (int)(L.*c.local).size();
    return 0;
}

using WindowFor = std::function<void(const std::function<void(int)>&)>;  // the pack's host threads over the windows of the batch

// One window on its way into the batch: what every pass of the layout reads, and what a pass leaves for the ones behind it.
struct WinPack {
    const int w;
    const limo_ba_window& W;
    const WindowProblem& pr;
    const PackOptions& po;
    PackedBatch& P;
    WinDesc& d;
    WinLists& L;
    const std::vector<int>& view_pad_off;  // evaluate-only batches: offset of every view's 64-aligned segment inside the window
    const int NS;                          // landmark shards
    const bool host_pairs;                 // P.pair_m is filled
    // from permute_landmarks on:
    std::vector<int> perm;    // caller's landmark -> packed landmark (local)
    std::vector<int> seg;     // start of every run of the packed order, and the end of the last
    std::vector<int> seg_of;  // run index of a packed landmark
    int n_var = 0, n_gp_var = 0;  // variable landmarks; those of them with a ground-plane row

    bool fail(const char* msg) {
        L.err = msg;
        L.rc = LIMO_ERR_INVALID;
        return false;
    }
};

bool pairs_on_host(const PackOptions& po) {  // (an evaluate-only batch has no reader of the planes)
    return po.host_pair_planes && !po.evaluate_only;
}

// lm_slot, and the measurements at the pair's index (kba_layout.hpp:BatchView::pair_m), of the window's landmarks: no pair yet
void clear_pair_tables(WinPack& c) {
    PackedBatch& P = c.P;
    const size_t n_pair = P.lm_slot.size();
    for (int v = 0; v < std::max(1, P.Vmax); ++v) std::fill_n(P.lm_slot.data() + (size_t)v * P.SL + c.d.lm0, c.W.n_lm, -1);
    if (c.host_pairs)
        for (int v = 0; v < std::max(1, P.Vmax); ++v) {
            std::fill_n(P.pair_m.data() + (size_t)v * P.SL + c.d.lm0, c.W.n_lm, 0.0f);
            std::fill_n(P.pair_m.data() + n_pair + (size_t)v * P.SL + c.d.lm0, c.W.n_lm, 0.0f);
            std::fill_n(P.pair_m.data() + 2 * n_pair + (size_t)v * P.SL + c.d.lm0, c.W.n_lm, kPairMissing);
        }
}

void copy_keyframes(WinPack& c) {
    PackedBatch& P = c.P;
    const limo_ba_window& W = c.W;
    const WinDesc& d = c.d;
    std::memcpy(P.pose.data() + (size_t)d.kf0 * 7, W.kf_pose, sizeof(double) * 7 * W.n_kf);
    std::memcpy(P.pdir.data() + (size_t)d.kf0 * 3, W.kf_plane_dir, sizeof(double) * 3 * W.n_kf);
    std::memcpy(P.pdist.data() + d.kf0, W.kf_plane_dist, sizeof(double) * W.n_kf);
    for (int k = 0; k < W.n_kf; ++k) P.kf_win[d.kf0 + k] = c.w;
}

// Packed landmark order: plain landmarks, then ground-plane landmarks (a Schur tile of plain landmarks then only touches the pose
// slots of the reduced camera system); inside each class by owning shard (landmark id mod n_shards), then input order.
// seg[] = start of every run of one (class, shard): with n_shards > 1 no workgroup straddles a run, so every workgroup has exactly
// one owner.  Constant landmarks (PackOptions::lm_fixed) come behind all of them, in input order, as one more run: a landmark
// workgroup is variable or constant as a whole (kba_kernels.hip:lin_lm_block), and the Schur blocks end where the run starts.
bool permute_landmarks(WinPack& c) {
    PackedBatch& P = c.P;
    const limo_ba_window& W = c.W;
    WinDesc& d = c.d;
    const int NS = c.NS, n_const = c.pr.n_const;
    const std::vector<uint8_t>& cst = c.pr.lm_const;
    if (n_const && NS > 1)  // (a guard: no entry point of the library sets both - limo_ba_solve_sharded takes no flags)
        return c.fail("constant landmarks in a landmark-sharded batch");
    std::vector<uint8_t> has_gp(W.n_lm, 0);
    for (const WindowProblem::GpRow& g : c.pr.gp) {
        has_gp[g.lm] = 1;
        c.n_gp_var += !cst[g.lm];
    }
    c.n_var = W.n_lm - n_const;
    c.perm.resize(W.n_lm);
    int nxt = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int r = 0; r < NS; ++r) {
            const int before = nxt;
            for (int l = 0; l < W.n_lm; ++l)
                if (!cst[l] && has_gp[l] == pass && l % NS == r) c.perm[l] = nxt++;
            if (NS > 1 && nxt > before) c.seg.push_back(before);
        }
    for (int l = 0; l < W.n_lm && n_const; ++l)
        if (cst[l]) c.perm[l] = nxt++;
    if (c.seg.empty()) c.seg.push_back(0);
    if (n_const && c.n_var > 0) c.seg.push_back(c.n_var);
    c.seg.push_back(W.n_lm);
    d.lm_gp0 = d.lm0 + c.n_var - c.n_gp_var;
    d.n_lm_const = n_const;
    c.seg_of.assign(W.n_lm, 0);
    for (size_t si = 0; si + 1 < c.seg.size(); ++si)
        for (int l = c.seg[si]; l < c.seg[si + 1]; ++l) c.seg_of[l] = (int)si;
    for (int l = 0; l < W.n_lm; ++l) {
        const int g = d.lm0 + c.perm[l];
        P.lm_win[g] = c.w;
        P.lm_id[g] = l;
        P.lm_weight[g] = W.lm_weight[l];
        P.lm_state[g] = c.pr.lm_state[l];
        P.lm_gp[g] = -1;  // (place_gp_rows)
        for (int i = 0; i < 3; ++i) P.lm[(size_t)g * 3 + i] = W.lm_pos[3 * l + i];
    }
    return true;
}

// the views' keyframes and camera constants: focal length and principal point, the rotation of the extrinsics, their translation
void place_views(WinPack& c) {
    PackedBatch& P = c.P;
    const WinDesc& d = c.d;
    for (int v = 0; v < d.n_view; ++v) {
        const int gv = d.view0 + v;
        P.view_kf[gv] = d.kf0 + c.pr.views[v].kf;
        P.view_win[gv] = c.w;
        const double* cam = c.W.cam + 10 * c.pr.views[v].cam;
        double* vc = P.view_cam.data() + (size_t)gv * 16;
        vc[0] = cam[0];
        vc[1] = cam[1];
        vc[2] = cam[2];
        quat_R(cam + 3, vc + 4);
        vc[13] = cam[7];
        vc[14] = cam[8];
        vc[15] = cam[9];
    }
}

// Observations sorted by (view, packed landmark), cut into blocks, and entered at their pair's index (lm_slot, pair_m).
bool place_observations(WinPack& c) {
    PackedBatch& P = c.P;
    const limo_ba_window& W = c.W;
    WinDesc& d = c.d;
    WinLists& L = c.L;
    const std::vector<int>& obs_view = c.pr.obs_view;
    const std::vector<int>& perm = c.perm;
    const size_t n_pair = P.lm_slot.size();
    // A (view, landmark) pair occurs at most once in a valid window, so the order is a placement: a dense table
    // [view][packed landmark] -> observation, read out row by row (a comparison sort of the ~9000 observations of a C2 window
    // through two indirections was the pack's hot spot: 0.5 ms per window and host thread).  Duplicates (rejected below) keep
    // their input order behind the first one.
    std::vector<int> order(W.n_obs);
    {
        std::vector<int> first((size_t)std::max(1, d.n_view) * std::max(1, W.n_lm), -1);
        bool dup = false;
        for (int i = 0; i < W.n_obs; ++i) {
            int& cell = first[(size_t)obs_view[i] * W.n_lm + perm[W.obs_lm[i]]];
            if (cell < 0)
                cell = i;
            else
                dup = true;
        }
        if (!dup) {
            int nxt = 0;
            for (size_t q = 0; q < first.size(); ++q)
                if (first[q] >= 0) order[nxt++] = first[q];
        } else {  // (an invalid window: the plain stable sort puts the duplicates side by side for the check below)
            std::iota(order.begin(), order.end(), 0);
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
                if (obs_view[a] != obs_view[b]) return obs_view[a] < obs_view[b];
                return perm[W.obs_lm[a]] < perm[W.obs_lm[b]];
            });
        }
    }
    d.blk0 = (int)L.blk_view.size();
    int pos = 0;
    for (int v = 0; v < d.n_view; ++v) {
        const int start = pos;
        while (pos < W.n_obs && obs_view[order[pos]] == v) ++pos;
        auto packed_at = [&](int i) { return d.obs0 + (c.po.evaluate_only ? c.view_pad_off[v] + (i - start) : i); };
        for (int b0 = start; b0 < pos;) {  // blocks of up to kObsBlock observations; none straddles a run of the landmark order
            int b1 = std::min(pos, b0 + kObsBlock);
            const int s0 = c.seg_of[perm[W.obs_lm[order[b0]]]];
            for (int i = b0 + 1; i < b1; ++i)
                if (c.seg_of[perm[W.obs_lm[order[i]]]] != s0) {
                    b1 = i;
                    break;
                }
            const int gkf = d.kf0 + c.pr.views[v].kf;
            if (P.kf_nblk[gkf] == 0) P.kf_blk0[gkf] = (int)L.blk_view.size();
            P.kf_nblk[gkf]++;
            L.blk_view.push_back(d.view0 + v);
            L.blk_obs0.push_back(packed_at(b0));
            L.blk_n.push_back(b1 - b0);
            L.blk_owner.push_back(W.obs_lm[order[b0]] % c.NS);
            b0 = b1;
        }
        for (int i = start; i < pos; ++i) {
            const int src = order[i];
            const int o = packed_at(i);
            const int l = perm[W.obs_lm[src]];
            P.obs_lm[o] = d.lm0 + l;
            P.obs_u[o] = W.obs_u[src];
            P.obs_v[o] = W.obs_v[src];
            P.obs_d[o] = W.obs_d[src];
            P.obs_src[o] = src;
            const size_t r = (size_t)v * P.SL + d.lm0 + l;
            if (P.lm_slot[r] != -1) return c.fail("duplicate (keyframe, landmark, camera) observation");
            P.lm_slot[r] = o;
            if (c.host_pairs) {  // the pair's measurement at the pair's index; the plane's depth is canonical (kPairNoDepth)
                P.pair_m[r] = W.obs_u[src];
                P.pair_m[n_pair + r] = W.obs_v[src];
                P.pair_m[2 * n_pair + r] = W.obs_d[src] > 0.0f ? W.obs_d[src] : kPairNoDepth;
            }
        }
        if (c.po.evaluate_only) {  // the padding behind the view's observations: inert entries
            for (int o = d.obs0 + c.view_pad_off[v] + (pos - start); o < d.obs0 + c.view_pad_off[v + 1]; ++o) {
                P.obs_lm[o] = d.lm0;
                P.obs_u[o] = P.obs_v[o] = 0.0f;
                P.obs_d[o] = -1.0f;
                P.obs_src[o] = -1;
            }
        }
    }
    d.n_blk = (int)L.blk_view.size() - d.blk0;
    return true;
}

// ground-plane rows sorted by keyframe (stable in landmark order), so each keyframe owns a contiguous range
void place_gp_rows(WinPack& c) {
    PackedBatch& P = c.P;
    WinDesc& d = c.d;
    WinLists& L = c.L;
    d.gp0 = (int)L.gp_lm.size();
    std::vector<WindowProblem::GpRow> rows(c.pr.gp);
    std::stable_sort(rows.begin(), rows.end(), [](const WindowProblem::GpRow& a, const WindowProblem::GpRow& b) { return a.kf < b.kf; });
    for (const WindowProblem::GpRow& g : rows) {
        const int gi = (int)L.gp_lm.size();
        if (P.kf_ngp[d.kf0 + g.kf] == 0) P.kf_gp0[d.kf0 + g.kf] = gi;
        P.kf_ngp[d.kf0 + g.kf]++;
        P.lm_gp[d.lm0 + c.perm[g.lm]] = gi;
        L.gp_lm.push_back(d.lm0 + c.perm[g.lm]);
        L.gp_kf.push_back(d.kf0 + g.kf);
        L.gp_w.push_back(g.w);
        L.gp_owner.push_back(g.lm % c.NS);
    }
    d.n_gp = (int)L.gp_lm.size() - d.gp0;
}

// the problem's scalars, as the kernels read them from the window's record
void describe_problem(WinPack& c) {
    WinDesc& d = c.d;
    const WindowProblem& pr = c.pr;
    d.n_depth = pr.n_depth;
    d.n_repr = pr.n_repr;
    d.do_trim = pr.do_trim ? 1 : 0;
    d.has_scale_reg = pr.has_scale_reg ? 1 : 0;
    d.scale_w = pr.scale_w;
    d.scale_s0 = pr.scale_s0;
    d.has_gp_reg = pr.has_gp_reg ? 1 : 0;
    d.speed_w = pr.speed_w;
    d.speed_dt = pr.speed_dt;
    std::memcpy(d.speed_vel, pr.speed_vel, sizeof(d.speed_vel));
    std::memcpy(d.speed_Rb, pr.speed_Rb, sizeof(d.speed_Rb));
    std::memcpy(d.speed_tb, pr.speed_tb, sizeof(d.speed_tb));
}

// present / free masks of the window's camera slots, and the compact numbering of the free ones: every pose slot first, then the
// plane slots (kba_layout.hpp, WinDesc::nfq)
void number_free_slots(WinPack& c) {
    PackedBatch& P = c.P;
    WinDesc& d = c.d;
    std::copy_n(c.pr.present.begin(), d.nc, P.cpresent.begin() + d.cam0);
    std::copy_n(c.pr.free.begin(), d.nc, P.cmask.begin() + d.cam0);
    const uint8_t* freem = P.cmask.data() + (size_t)d.cam0;
    d.nf = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i < d.nc; ++i)
            if (freem[i] && ((i % kCamSlots) >= 6) == (pass == 1)) P.cslot[(size_t)d.cam0 + i] = d.nf++;
        if (pass == 0) d.nfq = d.nf;
    }
    d.nf_pad = (d.nf + 1 + 15) / 16 * 16;  // + the rhs column
}

// workgroup tables: landmark workgroups of kBlock landmarks inside every run, Schur blocks of kSchurLmPerBlock variable landmarks
void build_workgroup_tables(WinPack& c) {
    const PackedBatch& P = c.P;
    WinDesc& d = c.d;
    WinLists& L = c.L;
    const std::vector<int>& seg = c.seg;
    d.lblk0 = (int)L.lblk_win.size();
    for (size_t si = 0; si + 1 < seg.size(); ++si)
        for (int l0 = seg[si]; l0 < seg[si + 1]; l0 += kBlock) {
            L.lblk_win.push_back(c.w);
            L.lblk_lm0.push_back(d.lm0 + l0);
            L.lblk_n.push_back(std::min(kBlock, seg[si + 1] - l0));
            L.lblk_owner.push_back(P.lm_id[d.lm0 + l0] % c.NS);
        }
    d.n_lblk = (int)L.lblk_win.size() - d.lblk0;
    d.sblk0 = (int)L.sblk_win.size();
    d.n_sblk_plain = 0;
    if (!c.po.pose_only && !c.po.evaluate_only && d.nf > 0) {
        const int per = kSchurLmPerBlock;
        // no Schur block straddles a shard run or the plain / ground-plane boundary, and none reaches into the constant run
        const int n_var = c.n_var, n_plain = n_var - c.n_gp_var;
        std::vector<int> cuts;
        for (int v : seg)
            if (v < n_var) cuts.push_back(v);
        cuts.push_back(n_plain);
        cuts.push_back(n_var);
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        for (size_t si = 0; si + 1 < cuts.size(); ++si)
            for (int l0 = cuts[si]; l0 < cuts[si + 1]; l0 += per) {
                L.sblk_win.push_back(c.w);
                L.sblk_lm0.push_back(d.lm0 + l0);
                L.sblk_n.push_back(std::min(per, cuts[si + 1] - l0));
                L.sblk_owner.push_back(P.lm_id[d.lm0 + l0] % c.NS);
                if (l0 < n_plain) d.n_sblk_plain++;
            }
    }
    d.n_sblk = (int)L.sblk_win.size() - d.sblk0;
}

// fast Schur variant (kba_kernels.hip): <= 4 keyframes with a free slot, one view per keyframe
void classify_schur(WinPack& c) {
    WinDesc& d = c.d;
    const std::vector<WindowProblem::View>& views = c.pr.views;
    const uint8_t* freem = c.P.cmask.data() + (size_t)d.cam0;
    d.schur_fast = 1;
    d.n_fk = 0;
    for (int q = 0; q < 4; ++q) d.fk[q] = d.fk_view[q] = -1;
    for (int k = 0; k < c.W.n_kf; ++k) {
        int nv = 0, view = -1;
        for (int v = 0; v < d.n_view; ++v)
            if (views[v].kf == k) {
                ++nv;
                view = d.view0 + v;
            }
        if (nv > 1) d.schur_fast = 0;
        if (freem[k * kCamSlots] || freem[k * kCamSlots + 6]) {
            if (d.n_fk < 4) {
                d.fk[d.n_fk] = k;
                d.fk_view[d.n_fk] = view;
            }
            d.n_fk++;
        }
    }
    if (d.n_fk > 4) d.schur_fast = 0;
    d.n_view_fixed0 = 0;  // leading views whose keyframe has no free pose block
    while (d.n_view_fixed0 < d.n_view && !freem[views[d.n_view_fixed0].kf * kCamSlots]) d.n_view_fixed0++;
    if (c.po.evaluate_only) d.n_view_fixed0 = 0;
}

// ---- the batch-level steps

// Every window's place in the fixed-size arrays (running sums over the windows) and the totals.  Evaluate-only batches: every
// view's observations start on a multiple of 64 (k_evaluate: a wave takes an ALIGNED range of 64 observations of ONE view; landmark
// order inside a view as everywhere: the landmark gathers of a wave stay inside ~1.5 KB).  The padding entries are inert
// observations (src -1, no depth) that no wave stores anything for.  (Tried and dropped: the view's depth observations first, so
// that a wave's depth rows are 64 aligned entries - the depth planes then cost what their bytes say, but every wave's gather spans
// twice the landmarks and the pass as a whole got 4 % slower: profiles/r06_experiment_evaluate_store_path.txt.)
void size_batch(const limo_ba_window* windows, const std::vector<WindowProblem>& probs, const PackOptions& po, PackedBatch& P,
                std::vector<std::vector<int>>& view_pad_off) {
    for (int w = 0; w < P.n_win; ++w) {
        const limo_ba_window& W = windows[w];
        const int nv = (int)probs[w].views.size();
        P.Vmax = std::max(P.Vmax, nv);
        WinDesc& d = P.win[w];
        std::memset(&d, 0, sizeof(d));
        d.kf0 = P.TK;
        d.n_kf = W.n_kf;
        d.lm0 = P.TL;
        d.n_lm = W.n_lm;
        d.view0 = P.TV;
        d.n_view = nv;
        d.obs0 = P.TO;
        d.n_obs = W.n_obs;
        if (po.evaluate_only) {
            std::vector<int>& vo = view_pad_off[w];
            vo.assign(nv + 1, 0);
            for (int i = 0; i < W.n_obs; ++i) vo[probs[w].obs_view[i] + 1]++;
            for (int v = 0; v < nv; ++v) vo[v + 1] = vo[v] + (int)pad64(vo[v + 1]);
            d.n_obs = vo[nv];
        }
        d.nc = W.n_kf * kCamSlots;
        d.nc_pad = (d.nc + 15) / 16 * 16;
        d.cam0 = d.kf0 * kCamSlots;
        d.pose_only = po.pose_only ? 1 : 0;
        P.TK += W.n_kf;
        P.TL += W.n_lm;
        P.TV += nv;
        P.TO += d.n_obs;
    }
    // + kObsBlock of slack behind the last observation (the stride of an evaluate-only batch's planes): no kernel of today stores
    // there - k_evaluate masks the lanes past a block's end
    P.SO = pad64(std::max(1, P.TO)) + kObsBlock;
    P.SL = pad64(std::max(1, P.TL));
}

// The fixed-size arrays.  The big ones stay uninitialised (kba_pack.hpp:uvec): the layout of a window writes every entry of the
// window's ranges (first touch by the thread that fills the window); the padding behind the last window is written here.
void allocate_arrays(const PackOptions& po, PackedBatch& P) {
    P.pose.resize((size_t)P.TK * 7);
    P.pdir.resize((size_t)P.TK * 3);
    P.pdist.resize(P.TK);
    P.kf_win.resize(P.TK);
    P.kf_blk0.assign(std::max(1, P.TK), 0);
    P.kf_nblk.assign(std::max(1, P.TK), 0);
    P.kf_gp0.assign(std::max(1, P.TK), 0);
    P.kf_ngp.assign(std::max(1, P.TK), 0);
    P.cmask.assign((size_t)P.TK * kCamSlots, 0);
    P.cpresent.assign((size_t)P.TK * kCamSlots, 0);
    P.cslot.assign((size_t)std::max(1, P.TK) * kCamSlots, -1);
    P.lm.resize((size_t)P.TL * 3);
    P.lm_win.resize(P.TL);
    P.lm_id.resize(P.TL);
    P.lm_gp.resize(P.TL);
    P.lm_weight.resize(P.TL);
    P.lm_state.resize(P.TL);
    P.lm_slot.resize((size_t)std::max(1, P.Vmax) * P.SL);
    for (int v = 0; v < std::max(1, P.Vmax); ++v)
        for (int64_t l = P.TL; l < P.SL; ++l) P.lm_slot[(size_t)v * P.SL + l] = -1;
    const size_t n_pair = P.lm_slot.size();
    P.pair_m.clear();
    if (pairs_on_host(po)) {
        P.pair_m.resize(3 * n_pair);
        for (int v = 0; v < std::max(1, P.Vmax); ++v)
            for (int64_t l = P.TL; l < P.SL; ++l) {
                P.pair_m[(size_t)v * P.SL + l] = P.pair_m[n_pair + (size_t)v * P.SL + l] = 0.0f;
                P.pair_m[2 * n_pair + (size_t)v * P.SL + l] = kPairMissing;
            }
    }
    P.view_kf.resize(P.TV);
    P.view_win.resize(P.TV);
    P.view_cam.assign((size_t)P.TV * 16, 0.0);
    P.obs_lm.resize(P.TO);
    P.obs_u.resize(P.TO);
    P.obs_v.resize(P.TO);
    P.obs_d.resize(P.TO);
    P.obs_src.resize(P.TO);
}

// Merge: local lists -> global lists, local indices -> global indices.  A serial pass fixes every window's place in the global
// lists (running sums) and the sizes; the copies and the index shifts of the windows then run on the host threads (2000 landmark
// entries per window to shift: this was 4.5 ms of a 1024-window create as one loop).
void merge_lists(const WindowFor& for_windows, std::vector<WinLists>& locals, PackedBatch& P) {
    using Base = std::array<int, kListKinds>;
    std::vector<Base> base(P.n_win);
    Base run{};
    for (int w = 0; w < P.n_win; ++w) {
        base[w] = run;
        for (int k = 0; k < kListKinds; ++k) run[k] += list_count(locals[w], (ListKind)k);
        WinDesc& d = P.win[w];
        d.blk0 += base[w][kObsBlocks];
        d.lblk0 += base[w][kLmBlocks];
        d.sblk0 += base[w][kSchurBlocks];
        d.gp0 += base[w][kGpRows];
    }
    for (const auto& col : kIntColumns) (P.*col.global).resize(run[col.kind]);
    for (const auto& col : kDoubleColumns) (P.*col.global).resize(run[col.kind]);
    for_windows([&](int w) {
        WinLists& L = locals[w];
        const WinDesc& d = P.win[w];
        const Base& bs = base[w];
        for (int k = d.kf0; k < d.kf0 + d.n_kf; ++k) {
            if (P.kf_nblk[k]) P.kf_blk0[k] += bs[kObsBlocks];
            if (P.kf_ngp[k]) P.kf_gp0[k] += bs[kGpRows];
        }
        for (int l = d.lm0; l < d.lm0 + d.n_lm; ++l)
            if (P.lm_gp[l] >= 0) P.lm_gp[l] += bs[kGpRows];
        for (const auto& col : kIntColumns) std::copy((L.*col.local).begin(), (L.*col.local).end(), (P.*col.global).begin() + bs[col.kind]);
        for (const auto& col : kDoubleColumns) std::copy((L.*col.local).begin(), (L.*col.local).end(), (P.*col.global).begin() + bs[col.kind]);
        L = WinLists();
    });
    P.TG = (int)P.gp_lm.size();
    P.SG = pad64(std::max(1, P.TG));
    P.n_blk = (int)P.blk_view.size();
    P.n_lblk = (int)P.lblk_win.size();
    P.n_sblk = (int)P.sblk_win.size();
}

// every window's place in the solve's scratch buffers, and their totals
void place_scratch(PackedBatch& P) {
    for (WinDesc& d : P.win) {
        d.hcc_off = P.hcc_total;
        P.hcc_total += (int64_t)d.nc * d.nc;
        d.spart_off = P.spart_total;
        P.spart_total += (int64_t)d.n_sblk * ((int64_t)d.nf_pad * d.nf_pad);
        d.sred_off = P.sred_total;
        if (P.n_shards > 1) P.sred_total += (int64_t)P.n_shards * schur_need_pad(d.nf);  // packed: upper triangle + rhs only
        d.xlv_off = P.xlv_total;
        P.xlv_total += (int64_t)d.n_view * kLinPartial;
        d.lvpart_off = P.lvpart_total;
        P.lvpart_total += (int64_t)d.n_lblk * d.n_view * kLinPartial;
        // camera system too large for LDS: scratch in global memory (kba_items.hpp:kCamLdsCapBytes)
        const int need = cam_class_doubles(d.nc, d.n_view);  // (not the solve's present, smaller scratch: no window changes class)
        d.cam_scr_off = -1;
        if (need * (int)sizeof(double) > kCamLdsCapBytes) {
            d.cam_scr_off = P.camscr_total;
            P.camscr_total += need;
        }
    }
}

// What a lean Schur wave needs to know about the group that starts at a block (spans of an unsharded batch).  Ground-plane groups
// are classified narrow / wide where the batch's ground-plane tile has three panels - schur_gp_panels, the rule of
// kba_batch_plan.hpp:plan_batch - and nowhere else: two panels are what a narrow wave runs anyway.
void build_schur_groups(const WindowFor& for_windows, PackedBatch& P) {
    P.sgrp.assign((size_t)P.n_sblk, SchurGroup{});
    const bool classify = schur_gp_panels(P.win) >= 3;
    for_windows([&](int w) {
        const WinDesc& d = P.win[w];
        if (!d.schur_fast) return;
        for (int sb = d.sblk0; sb < d.sblk0 + d.n_sblk; ++sb)
            P.sgrp[sb] = schur_group_make(d, w, sb, kSchurSpan, kSchurSpanGp, P.sblk_lm0.data(), P.sblk_n.data(), P.cslot.data(),
                                          classify ? P.lm_gp.data() : nullptr, classify ? P.gp_kf.data() : nullptr);
    });
    P.n_sgrp_narrow = P.n_sgrp_wide = 0;
    if (classify)
        for (const WinDesc& d : P.win) {
            if (!d.schur_fast) continue;
            for (int i = d.n_sblk_plain; i < d.n_sblk; i += kSchurSpanGp) (P.sgrp[d.sblk0 + i].gp_class == kSchurGpWide ? P.n_sgrp_wide : P.n_sgrp_narrow)++;
        }
}

// Evaluate-only batches.  The materialised pass (k_evaluate) writes the rows that EXIST: the depth rows go into COMPACT planes over
// the depth observations only, indexed by the observation's rank among them in packed order (obs_rank).  Its work items are
// wave-sized: an aligned range of 64 observations of one observation block (= one view), each knowing the rank of its first depth
// observation.  A wave loads base + lane whatever the block's length, so every block must start on the 64-grid of its view's padded
// segment (false otherwise): views are aligned (size_batch) and the blocks inside one are kObsBlock apart - unless a block is cut
// at a run of the landmark order, which only a sharded batch has (refused by pack_windows).
bool build_eval_chunks(PackedBatch& P) {
    P.echunk.clear();
    P.obs_rank.assign((size_t)std::max(1, P.TO), -1);
    std::vector<int32_t> before((size_t)P.TO + 1, 0);  // depth observations in front of observation o
    for (int o = 0; o < P.TO; ++o) {
        const bool dep = P.obs_d[o] > 0.0f;
        if (dep) P.obs_rank[o] = before[o];
        before[o + 1] = before[o] + (dep ? 1 : 0);
    }
    P.TD = before[P.TO];
    P.SD = pad64(std::max(1, P.TD)) + 64;
    for (int b = 0; b < P.n_blk; ++b) {
        const int o0 = P.blk_obs0[b], o1 = o0 + P.blk_n[b];
        if ((o0 & 63) != 0) return false;
        for (int a = o0; a < o1; a += 64) {
            EvalChunk ch;
            ch.base = a;
            ch.view = P.blk_view[b];
            ch.o0 = o0;
            ch.o1 = o1;
            ch.dep0 = before[a];
            ch.pad = 0;
            P.echunk.push_back(ch);
        }
    }
    P.n_echunk = (int)P.echunk.size();
    return true;
}

}  // namespace

int pack_windows(int32_t n, const limo_ba_window* windows, const limo_ba_options& opts, const PackOptions& po,
                 PackedBatch& P, std::string& err) {
    if (n <= 0 || !windows) {
        err = "no windows";
        return LIMO_ERR_INVALID;
    }
    if (po.evaluate_only && po.shards > 1) {  // (build_eval_chunks; no entry point of the library sets both)
        err = "evaluate-only batch with landmark shards";
        return LIMO_ERR_INVALID;
    }
    auto name_window = [&](int w, const std::string& msg) { return po.per_window_prior ? "window " + std::to_string(w) + ": " + msg : msg; };
    using Clock = std::chrono::steady_clock;
    auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t_p0 = Clock::now();
    P = PackedBatch();
    P.n_win = n;
    P.n_shards = std::max(1, po.shards);
    P.evaluate_only = po.evaluate_only;
    P.win.resize(n);
    // host threads over the windows
    // (1024 C2 windows on the 256-thread host of an MI355X box: fill 15.5 ms with 16 threads, 6.5 ms with 64, no gain beyond)
    const WindowFor for_windows = [&](const std::function<void(int)>& f) { pack_parallel_for(n, std::min(64u, (unsigned)((n + 7) / 8)), 1, f); };

    // 1. the rules: every window's problem, in the caller's indices
    std::vector<WindowProblem> probs(n);
    for_windows([&](int w) { probs[w] = build_window_problem(windows[w], opts, po, w); });
    for (int w = 0; w < n; ++w)
        if (probs[w].rc != LIMO_OK) {
            err = name_window(w, probs[w].err);
            return probs[w].rc;
        }
    // 2. every window's place in the fixed-size arrays; 3. the arrays
    std::vector<std::vector<int>> view_pad_off(n);
    size_batch(windows, probs, po, P, view_pad_off);
    const auto t_p0b = Clock::now();
    allocate_arrays(po, P);
    const auto t_p1 = Clock::now();
    // 4. the layout of every window: its ranges of the arrays, its lists with local indices
    std::vector<WinLists> locals(n);
    for_windows([&](int w) {
        WinPack c{w, windows[w], probs[w], po, P, P.win[w], locals[w], view_pad_off[w], P.n_shards, pairs_on_host(po)};
        clear_pair_tables(c);
        copy_keyframes(c);
        if (!permute_landmarks(c)) return;
        place_views(c);
        if (!place_observations(c)) return;
        place_gp_rows(c);
        describe_problem(c);
        number_free_slots(c);
        build_workgroup_tables(c);
        classify_schur(c);
    });
    const auto t_p2 = Clock::now();
    for (int w = 0; w < n; ++w)
        if (locals[w].rc != LIMO_OK) {
            err = name_window(w, locals[w].err);
            return locals[w].rc;
        }
    // 5. the lists of the batch; 6. the windows' places in the solve's scratch
    merge_lists(for_windows, locals, P);
    place_scratch(P);
    if (std::getenv("KBA_PACK_TRACE"))
        std::fprintf(stderr, "[kba] pack: views + sizes %.1f ms, arrays %.1f ms, fill %.1f ms, merge %.1f ms\n", ms(t_p0, t_p0b), ms(t_p0b, t_p1),
                     ms(t_p1, t_p2), ms(t_p2, Clock::now()));
    // 7. the Schur group records; 8. the evaluate chunks
    build_schur_groups(for_windows, P);
    if (P.evaluate_only && !build_eval_chunks(P)) {
        err = "evaluate-only batch: an observation block does not start on a multiple of 64";
        return LIMO_ERR_INVALID;
    }
    return LIMO_OK;
}

void run_schedule(Executor& ex, const limo_ba_options& o) {
    using Clock = std::chrono::steady_clock;
    auto run_solve = [&](int max_iter, int select) {
        ex.solve_init(max_iter, select);
        const auto t0 = Clock::now();
        for (;;) {
            ex.linearize();
            if (ex.active_count() == 0) break;
            if (o.max_solver_time_sec > 0.0 &&
                std::chrono::duration<double>(Clock::now() - t0).count() >= o.max_solver_time_sec) {
                ex.expire(0);
                break;
            }
            ex.step();
        }
    };
    for (int r = 0; r < o.num_trim_rounds; ++r) {
        run_solve(o.trim_solver_iterations, 1);
        run_solve(3 * o.trim_solver_iterations, 2);
        ex.trim();
    }
    run_solve(o.max_num_iterations, 0);
}

}  // namespace kba
