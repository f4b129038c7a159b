// kba_pack.hpp — host-side flattening of limo_ba_window[] into the batch layout of kba_layout.hpp, and the
// phase orchestration (solveTrimmed schedule) that drives an Executor (HIP kernels, or the test emulator).
//
// Replaces the host logic of BundleAdjusterKeyframes::solve()/adjustPoseOnly() that decides WHICH residuals and
// parameters exist (reference: keyframe_bundle_adjustment/src/bundle_adjuster_keyframes.cpp:498-562 ground-plane
// wiring, :704-736 scale / ground-plane regularisation and constness rules, :740-758 trimming schedule) and the
// outer loop of robust_optimization::solveTrimmed (robust_optimization/src/robust_solving.cpp:140-248).
#pragma once
#include <array>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "kba_layout.hpp"

namespace kba {

// std::vector whose resize() leaves trivially-constructible elements uninitialised: the big per-observation /
// per-landmark arrays are written exactly once by the (threaded) packing, zero-filling them first only costs a
// serial pass of page faults.
// The big arrays may come out of an ARENA the caller lends to one pack_windows call (the HIP library: a pinned host block the
// context keeps between batches - no page faults on first touch, and the upload is a DMA straight out of where the pack wrote).
// A bump allocator: requests of kPackArenaMin bytes or more are carved from it while it has room, everything else (and everything
// when no arena is lent) comes from the heap; memory of an arena is never freed piecewise - its owner recycles the block when the
// PackedBatch is gone (pack_arena_owns: deallocate() of such a pointer is a no-op).
struct PackArena {
    char* base = nullptr;
    size_t cap = 0, used = 0;
    size_t wanted = 0;  // bytes the arena-sized requests of this pack added up to (what the arena should hold next time)
};
constexpr size_t kPackArenaMin = 64u << 10;
void pack_arena_lend(PackArena* a);              // this thread's pack_windows carves from *a until pack_arena_lend(nullptr)
void pack_arena_register(const void* base, size_t cap, bool add);  // the ranges pack_arena_owns knows (process-wide)
bool pack_arena_owns(const void* p);
void* pack_arena_take(size_t bytes);             // nullptr: no arena lent / no room
// Lends *a (nothing when null) for the life of the guard: the loan ends however the scope is left, so that the thread's arena
// pointer never outlives the PackArena it aims at.
struct PackArenaLend {
    explicit PackArenaLend(PackArena* a) { pack_arena_lend(a); }
    ~PackArenaLend() { pack_arena_lend(nullptr); }
    PackArenaLend(const PackArenaLend&) = delete;
    PackArenaLend& operator=(const PackArenaLend&) = delete;
};

template <typename T>
struct default_init_allocator : std::allocator<T> {
    template <typename U>
    struct rebind {
        using other = default_init_allocator<U>;
    };
    T* allocate(size_t n) {
        const size_t bytes = n * sizeof(T);
        if (bytes >= kPackArenaMin)
            if (void* p = pack_arena_take(bytes)) return static_cast<T*>(p);
        return static_cast<T*>(::operator new(bytes));
    }
    void deallocate(T* p, size_t) noexcept {
        if (pack_arena_owns(p)) return;
        ::operator delete(p);
    }
    template <typename U>
    void construct(U* p) noexcept(std::is_nothrow_default_constructible<U>::value) {
        ::new (static_cast<void*>(p)) U;
    }
    template <typename U, typename... Args>
    void construct(U* p, Args&&... args) {
        ::new (static_cast<void*>(p)) U(std::forward<Args>(args)...);
    }
};
template <typename T>
using uvec = std::vector<T, default_init_allocator<T>>;

struct PackedBatch {
    int32_t n_win = 0, TK = 0, TL = 0, TO = 0, TV = 0, TG = 0, n_blk = 0, n_lblk = 0, n_sblk = 0, Vmax = 0;
    int64_t SO = 0, SL = 0, SG = 0;
    int64_t SD = 0;              // evaluate-only batches: stride of the COMPACT depth-row planes (depth observations only, kba_layout.hpp)
    int32_t TD = 0;              // ... and how many depth observations (d > 0) the batch has
    int64_t hcc_total = 0, spart_total = 0, sred_total = 0, camscr_total = 0, lvpart_total = 0, xlv_total = 0;
    bool evaluate_only = false;  // planes hold the full Jacobians instead of the factored form
    int32_t n_shards = 1;        // landmark shards; owner of landmark l = (caller's index of l) mod n_shards
    std::vector<int32_t> blk_owner, lblk_owner, sblk_owner, gp_owner;  // owning shard of every workgroup / gp row
    std::vector<WinDesc> win;
    std::vector<double> pose, pdir, pdist;  // initial parameters
    uvec<double> lm;
    std::vector<int32_t> kf_win, kf_blk0, kf_nblk, kf_gp0, kf_ngp;
    std::vector<uint8_t> cmask, cpresent;
    std::vector<int32_t> cslot;
    uvec<int32_t> lm_gp;
    uvec<int32_t> lm_win, lm_slot;
    uvec<int32_t> lm_id;  // packed landmark -> index in the caller's window
    uvec<double> lm_weight;
    uvec<uint8_t> lm_state;
    std::vector<int32_t> view_kf, view_win;
    std::vector<double> view_cam;
    std::vector<int32_t> blk_view, blk_obs0, blk_n;
    // evaluate-only batches: the wave-sized work items of k_evaluate (kba_layout.hpp:EvalChunk), n_echunk of them
    std::vector<EvalChunk> echunk;
    int32_t n_echunk = 0;
    std::vector<int32_t> obs_rank;  // evaluate-only batches: index of the observation's depth row in the depth planes or -1
    uvec<int32_t> obs_lm;
    uvec<float> obs_u, obs_v, obs_d;
    // the measurements u | v | d over lm_slot's entries, [3][lm_slot.size()] (kba_layout.hpp:BatchView::pair_m) - only with
    // PackOptions::host_pair_planes (the emulator); empty otherwise: the library fills the device planes itself (k_pair_fill)
    uvec<float> pair_m;
    uvec<int32_t> obs_src;  // packed observation -> index in the caller's window
    std::vector<int32_t> lblk_win, lblk_lm0, lblk_n, sblk_win, sblk_lm0, sblk_n;
    std::vector<SchurGroup> sgrp;  // [n_sblk] kba_layout.hpp:SchurGroup (fast-class windows; zero elsewhere)
    // ground-plane groups of fast-class windows by SchurGroup::gp_class, in a batch whose ground-plane tile has three panels (more
    // than 32 columns in some fast-class window); a batch of two panels or one classifies nothing: 0 / 0, every record wide
    int32_t n_sgrp_narrow = 0, n_sgrp_wide = 0;
    std::vector<int32_t> gp_lm, gp_kf;
    std::vector<double> gp_w;
};

struct PackOptions {
    bool pose_only = false;
    bool evaluate_only = false;  // no problem-build logic (no ground plane / regularisers), every parameter free
    const limo_speed_prior* prior = nullptr;
    int shards = 1;  // > 1: lay the batch out for landmark sharding (no workgroup straddles two shards); refused with evaluate_only
    // A batch of adjustPoseOnly problems (limo_ba_batch_create_pose_only): window w takes window_priors[w] (null: no window has a
    // prior; an entry with speed_weight <= 0: that window has none) instead of `prior`, and an invalid window is named by its index
    // in the error text.
    bool per_window_prior = false;
    const limo_speed_prior* window_priors = nullptr;
    // Solve windows with per-landmark constness (limo_ba_solve_fixed_landmarks): null, or one entry per window, each null or that
    // window's n_lm flags in the caller's landmark order - != 0: the landmark is a constant parameter block (lm_state 2).  The
    // flagged landmarks of a window form their own run of the packed order behind the variable ones (WinDesc::n_lm_const): landmark
    // workgroups of their own, no Schur block.  A window without a flag set packs exactly as it does without the array.
    const uint8_t* const* lm_fixed = nullptr;
    // Fill PackedBatch::pair_m on the host.  The library turns it off: 12 B x Vmax x SL would be written here and cross the bus,
    // where a kernel at create forms the planes from lm_slot and obs_u / obs_v / obs_d, which are on the device anyway.
    bool host_pair_planes = true;
};

// THE PROBLEM'S RULES: which residual and parameter blocks one window has - the reference's problem-build logic of
// BundleAdjusterKeyframes::solve() / adjustPoseOnly(), decided from the caller's window and the mode alone.
// Everything here is in the CALLER's indices (keyframe, landmark, observation, camera as the window numbers them); nothing knows of
// the batch or of a packed index.  pack_windows lays out what this says exists.
struct WindowProblem {
    int rc = LIMO_OK;           // validation: LIMO_OK, or the window is refused with err (a literal) and nothing below is meaningful
    const char* err = nullptr;
    struct View {
        int kf, cam;
    };
    std::vector<View> views;    // the (keyframe, camera) pairs that carry observations, in pack order (build_window_problem)
    std::vector<int> obs_view;  // [n_obs] the view of every observation (index into views)
    struct GpRow {
        int kf, lm;
        double w;
    };
    std::vector<GpRow> gp;          // ground-plane rows, in landmark order
    std::vector<uint8_t> lm_state;  // [n_lm] 0: not in the problem, 1: variable, 2: constant parameter block
    std::vector<uint8_t> lm_const;  // [n_lm] flagged in PackOptions::lm_fixed (whatever its state); n_const of them
    int n_const = 0;
    std::array<uint8_t, kMaxKf * kCamSlots> present{}, free{};  // [n_kf * kCamSlots] the camera slot's parameter exists / is variable
    bool has_scale_reg = false;     // PoseRegularization between the first two poses: weight and target
    double scale_w = 0.0, scale_s0 = 0.0;
    bool has_gp_reg = false;        // the ground-plane regularisers
    int n_depth = 0, n_repr = 0;    // residual blocks built: observations with a depth, all observations
    bool do_trim = false;           // the trimmed schedule applies (n_lm > min_landmarks_for_trimming)
    double speed_w = 0.0, speed_dt = 0.0, speed_vel[3] = {0, 0, 0}, speed_Rb[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0},
           speed_tb[3] = {0, 0, 0};  // SpeedRegularizationVector2 of a pose-only window; speed_w == 0: none
};
// w: the window's index in the batch - it selects the window's entry of PackOptions::window_priors / lm_fixed, nothing else.
WindowProblem build_window_problem(const limo_ba_window& W, const limo_ba_options& opts, const PackOptions& po, int w);

// Runs f(0 .. n - 1) on host threads, the caller among them: min(hardware threads, max_threads) of them - KBA_PACK_THREADS, read
// here and nowhere else, overrides the count - handing out `grain` consecutive items at a time; one thread or none: a plain loop.
// The threads are the pack's pool (kba_pack.cpp:PackPool), or fresh ones while another caller holds it.
void pack_parallel_for(int n, unsigned max_threads, int grain, const std::function<void(int)>& f);

// Returns LIMO_OK or a negative limo_status; err receives a message.
int pack_windows(int32_t n, const limo_ba_window* windows, const limo_ba_options& opts, const PackOptions& po,
                 PackedBatch& out, std::string& err);

SolveConsts make_consts(const limo_ba_options& o);

// One ceres-style solve phase / trimming step, implemented by the HIP library and by the test emulator.
struct Executor {
    virtual ~Executor() {}
    // select = 0: every window; 1: windows with do_trim; 2: of those, the ones whose last solve did not
    // reduce the cost (robust_solving.cpp:172-181)
    virtual void solve_init(int max_iter, int select) = 0;
    virtual void linearize() = 0;     // linearise windows that need it + IterationZero / successful-step tail
    virtual int active_count() = 0;   // number of windows still iterating (synchronises)
    virtual void step() = 0;          // trust-region step, candidate evaluation, accept / reject
    virtual void trim() = 0;          // quantile trimming of windows with do_trim
    virtual void expire(int) {}       // wall-clock cap reached: stop every active window (NO_CONVERGENCE)
};

// solveTrimmed schedule over a whole batch (all windows advance in lock-step, finished windows idle).
void run_schedule(Executor& ex, const limo_ba_options& o);

}  // namespace kba
