// limo_batch.hpp — the host object behind `limo_ba_batch*`.  limo_ba_batch is the batch itself (storage, reset image, kernel plan,
// the ONE launch site of every solver kernel) plus a value member for each thing that drives it:
//   run     SolveRun       the switches and counters of the solve in progress (value-initialised per solve)
//   lock    LockStep       the Executor of run_schedule: worklists, the ring of active counts          limo_batch_lockstep.hpp
//   shards  ShardExchange  the landmark-sharded solve: producer blocks, exchange steps, reductions     limo_batch_lockstep.hpp
//   stream  StreamSolve    slot groups, their streams and scheduler words                              limo_batch_stream.hpp
//   one     OneLaunch      k_solve_wg / k_solve_coop and the recovery of a barrier timeout             limo_batch_onelaunch.hpp
//   log     IterationLog   the per-window iteration log                                                 (this file)
//   cov     PoseCovariance the covariance pass behind a solve, its storage                              (this file)
//   timers  KernelTimers   event pairs around timed kernels, the clock of a solve                      (this file)
// Every struct declares all its data first, grouped by lifetime.  Included by limo_hip.hip alone (behind kba_kernels.hip and
// `using namespace kba`), which keeps the C ABI.
#pragma once
#include <cstddef>

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

// The batch's pinned block of 64 bytes, as the host and (d_pin) the device see it.
struct PinnedWords {
    int32_t active[4];  // LockStep: written by k_cam_assemble, read by the host one iteration later
    int32_t unused[4];
    int32_t coop_abort;  // OneLaunch: set by a barrier of k_solve_coop that was not met in time
    int32_t unused2[7];
};
static_assert(offsetof(PinnedWords, coop_abort) == 8 * sizeof(int32_t) && sizeof(PinnedWords) == 64, "the words k_cam_assemble and k_solve_coop write");

}  // namespace

// What limo_ba_batch_solve knows about the solve in progress beyond its results (limo_ba_batch::publish_run).
struct SolveRun {
    // ---- per solve: `run = {}` at its start
    SolveSwitches sw;
    int path = PATH_NONE;      // the path that ran (after a refused or timed-out cooperative launch: the launch sequence)
    bool coop_redone = false;  // a barrier of k_solve_coop timed out and the solve was redone
    int coop_G = 0;            // workgroups per window of the cooperative launch
    int64_t n_rounds = 0, n_pair_launches = 0;
    int64_t n_narrow_launches = 0, n_widegp_launches = 0;  // launches that ran narrow / three-panel ground-plane waves
    int lin_variant = 1;  // k_lin_lm<true> / <false> of the last launch; the one-launch kernels always linearise through LDS
    int64_t n_cam_launches[2][2] = {{0, 0}, {0, 0}};  // [assemble, solve][half, full]
};

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

// ---- lock-step solve: what run_schedule (kba_pack.hpp) drives
struct LockStep : Executor {
    limo_ba_batch& b;
    // ---- per batch
    std::vector<ViewLists> wl;  // [pv.size()]
    int32_t *d_act_blk = nullptr, *d_act_lblk = nullptr, *d_act_sblk = nullptr, *d_act_win = nullptr;  // device lists of a re-batched active set
    int32_t* d_flags = nullptr;
    int32_t* h_flags = nullptr;  // pinned
    size_t h_flags_bytes = 0;
    hipEvent_t act_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // PinnedWords::active[i] of an iteration is written
    // ---- per solve: set by solve_init
    int it_no = 0;
    bool first_lin = false, assemble_pending = false;

    explicit LockStep(limo_ba_batch& batch) : b(batch) {}
    int alloc();
    int create_events();
    void release_pinned();
    void destroy_events();
    int upload_list(const std::vector<int32_t>& v, const int32_t** out);
    int build_full_sblk(size_t i);
    void full_lists();
    void rebatch();
    void assemble(int iter);
    void solve_init(int max_iter, int select) override;
    void linearize() override;
    int active_count() override;
    void expire(int) override;
    void step() override;
    void trim() override;
};

// ---- landmark sharding.  n_shards == 1: everything is inert (pv = {bv}, local = {0}) and every method returns at once.
// Every shard holds the same global layout and owns the observation / landmark / Schur workgroups of its
// landmarks (rank lists); the per-workgroup partial arrays it produces live in its own "producer view" pv[i] and
// are summed into the consumer view bv before each window-level kernel: by RCCL all-reduce when the shards are
// ranks (one local shard), by k_sum_shards when all shards are virtual on this GPU.
struct ShardExchange {
    limo_ba_batch& b;
    // ---- per batch: fixed by batch_create_impl and setup
    int n_shards = 1, rank = 0;
    bool is_virtual = true;
    std::vector<int> local;
    ExchangeLayout xl;
    double* arena_c = nullptr;      // consumer view: the shards' contributions side by side (kba_buffers.hpp:exchange_layout)
    std::vector<double*> blocks;    // block of local shard i (what it contributes per LM iteration)
    std::vector<double*> trims;     // trimming arenas: [0] consumer, [1 + i] local shard i
    double* d_gather = nullptr;     // [world][block] staging of the all-gather
    WinDesc* d_win_orig = nullptr;  // the batch's own window descriptors (bv.win of the consumer view is modified)
    double* d_lm_tmp = nullptr;
    // ---- across solves
    int64_t n_exchanges = 0, exchange_bytes = 0;  // all-reduce calls / bytes of this batch so far (limo_ctx_exchange_stats)

    explicit ShardExchange(limo_ba_batch& batch) : b(batch) {}
    int setup();
    void reduce(int what, const int32_t* win, int n_win);
    void exchange(int point);
    void host_exchange(const double* src, double* dst, size_t count, int kind);
    void exchange_trim();
    int gather_landmarks();
};

// ---- streaming solve (device-side scheduler k_sched): windows move through n_slots slots, a finished window is
// replaced by the next pending one, so every launch round works on a full set (kba_kernels.hip:k_sched).
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
struct StreamSolve {
    limo_ba_batch& b;
    static constexpr int kSchurPairBound = 384;  // windows in flight in a slot group up to which a round launches the pair kernel (192: -0.7 %, 768: -9 % at 1024 windows)
    // ---- across solves: built by the first streaming solve, rebuilt when the number of groups changes (setup)
    std::vector<StreamGroup> groups;
    int groups_built = 0;
    int n_slots = 0;
    int32_t* d_sched_ctl = nullptr;  // [0] cursor over the batch's windows, [1] windows finished (shared by the groups)
    hipEvent_t start_ev = nullptr;

    explicit StreamSolve(limo_ba_batch& batch) : b(batch) {}
    void teardown();
    int setup(const StreamGeometry& geo);
    void enqueue_round(StreamGroup& g, int round, bool time_kernels, int in_flight_max);
    int solve();
};

// ---- a whole solve in ONE launch: k_solve_wg (a workgroup per window) and k_solve_coop (G workgroups per window that meet at
// device-wide barriers).  Which solve takes them: kba_batch_plan.hpp:choose_solve_path.
struct OneLaunch {
    limo_ba_batch& b;
    // ---- across solves: made by the first cooperative launch
    int32_t* d_coop_bar = nullptr;
    double* d_coop_red = nullptr;
    // ---- per solve: set by solve_coop, taken back by recover
    bool coop_launched = false;

    explicit OneLaunch(limo_ba_batch& batch) : b(batch) {}
    long long cap_ticks() const;
    void solve_wg();
    bool solve_coop(const CoopGeometry& geo);
    int recover();
};

// ---- iteration log (limo_hip.h:limo_ba_iteration; kba_lm.hpp:lm_log_push).  limo_ba_batch_solve binds it when the context's
// switch is on: every window gets the exact bound of the schedule as its capacity, the reset image carries the pointers (so
// limo_ba_batch_reset and a recovered barrier timeout start the log again at zero entries), k_log_bind puts them into the live state.
struct IterationLog {
    limo_ba_batch& b;
    // ---- across solves: grown by bind
    limo_ba_iteration* d_log = nullptr;
    int log_cap = 0;    // entries per window of the binding in force; 0: no log
    int log_alloc = 0;  // entries per window d_log has room for

    explicit IterationLog(limo_ba_batch& batch) : b(batch) {}
    static int bound(const limo_ba_options& o) {
        const int64_t t = std::max(0, o.trim_solver_iterations), r = std::max(0, o.num_trim_rounds), m = std::max(0, o.max_num_iterations);
        return (int)std::min<int64_t>(r * ((t + 1) + (3 * t + 1)) + (m + 1), 1 << 24);
    }
    int bind(bool on);
    int read(int w, int cap, limo_ba_iteration* out, int32_t* n);
    int export_to_ctx();
};

// ---- marginal pose covariance (limo_hip.h, "Pose covariance"; kba_items.hpp:cam_cov).  With the context's switch on every solve of
// the batch ends with run(): the LM state is saved, the lock-step train linearises every window once more at its final point with
// both clamp bounds of the damping at zero (k_view_consts, k_lin_lm, k_cam_assemble, the Schur launch over the full worklists, with
// the solve's own loss scales), k_cam_cov factors the undamped Schur complement, and the LM state is put back.  Everything else
// the train writes is scratch that the next linearisation of a solve writes again before it reads it.
struct PoseCovariance {
    limo_ba_batch& b;
    // ---- across solves: made by the first solve with the switch on (ensure)
    double* d_cov = nullptr;        // the windows' [6 n_kf]^2 matrices, back to back
    int32_t* d_status = nullptr;    // [n_win] LIMO_COV_*
    int64_t *d_cov_off = nullptr, *d_scr_off = nullptr;
    double* d_scratch = nullptr;    // cam_cov's scratch of the windows too large for LDS
    WinState* d_st_save = nullptr;
    WinRed* d_red_save = nullptr;
    std::vector<int64_t> cov_off;   // [n_win + 1]
    int lds_bytes = 0;
    bool ready = false;             // ensure() has made all of the above
    bool offered = true;            // false: the batch of a call that reports no covariance (limo_ba_solve_sharded) - no pass
    // ---- per solve
    bool computed = false;          // the last solve of the batch ended with the pass

    explicit PoseCovariance(limo_ba_batch& batch) : b(batch) {}
    int ensure();
    int run();
    int read(int w, int64_t cap, double* out, int32_t* status);
    int export_to_ctx();
};

// ---- kernel timing (linearisation, Schur) via HIP events on the stream of the launch, and the clock of a whole solve
struct KernelTimers {
    limo_ba_batch& b;
    // ---- across solves: accumulated until limo_ba_batch_kernel_stats resets them
    std::vector<EventPair> ev_pool;
    size_t ev_used = 0;
    double k_ms_acc[2] = {0.0, 0.0};  // indexed by LIMO_KERNEL_LINEARIZE / LIMO_KERNEL_SCHUR
    int64_t k_launches[2] = {0, 0};
    hipEvent_t ev_total_a = nullptr, ev_total_b = nullptr;
    double total_ms_acc = 0.0;
    // ---- per solve
    std::chrono::steady_clock::time_point t0;
    double last_solve_sec = 0.0;

    explicit KernelTimers(limo_ba_batch& batch) : b(batch) {}
    int create_events();
    void destroy_events();
    EventPair* timed(int kernel, hipStream_t on = nullptr);
    void stop(EventPair* ep, hipStream_t s);
    int start_solve();
    int stop_solve();
    int collect();
};

struct limo_ba_batch {
    // ---- per batch: fixed by batch_create_impl and upload
    limo_ctx* ctx = nullptr;
    PackedBatch P;
    bool holds_pack_arena = false;  // P's big arrays live in ctx->pack_arena
    bool pose_batch = false;        // made by limo_ba_batch_create_pose_only: limo_ba_batch_solve picks its launch path by that
    BatchView bv;
    std::vector<BatchView> pv;  // producer views: {bv}, or one per local shard (ShardExchange)
    std::vector<std::pair<void*, size_t>> allocs;  // device blocks of this batch (returned to the context's pool)
    double *d_plane_rep = nullptr, *d_plane_dep = nullptr;
    double *d_pose0 = nullptr, *d_pdir0 = nullptr, *d_pdist0 = nullptr, *d_lm0 = nullptr;  // the reset image ...
    uint8_t* d_lm_state0 = nullptr;
    std::vector<WinState> st0;  // ... and that of the LM state (IterationLog::bind puts the log pointers in)
    PinnedWords *h_pin = nullptr, *d_pin = nullptr;  // pinned; the same words as the device sees them
    BatchPlan plan;  // kernel variants and LDS sizes (kba_batch_plan.hpp) ...
    const void *schur_fn_plain = nullptr, *schur_fn_leangp = nullptr, *schur_fn_gen = nullptr;  // ... and the variants as kernels
    const void* schur_fn_narrow = nullptr;  // plan.narrow: k_schur_lean_gp
    bool schur_pair_ok = false;             // plan.pair_ok, and KBA_NO_SCHUR_PAIR is not set
    // lanes of the camera kernels (kba_batch_plan.hpp:plan_cam_lanes / cam_lanes_for_launch; limo_ctx_last_cam_lanes_info)
    CamOccupancy cam_occ;
    CamLanesPlan cam_plan;
    // ---- per solve call: the options of the last limo_ba_batch_solve and what follows from them, its status
    limo_ba_options opts;
    SolveConsts c;
    int rc = LIMO_OK;
    SolveRun run;
    // per-window options of the solve in progress (limo_ba_batch_solve_each with options that differ): the host's records, uploaded
    // to d_wopt (made by the first such solve); every view of a uniform solve holds a null table (set_window_table)
    std::vector<WinOpts> wopt_host;
    WinOpts* d_wopt = nullptr;
    // ---- across solves
    int lin_lds_set = 0;  // dynamic LDS k_lin_lm<false> was allowed beyond the default 48 KB (k_lin_lm<true> never needs more)
    // S_part holds packed slabs (SolveConsts::slab_packed) of an earlier solve of this batch.  The tile layout counts on the zeros of
    // the allocation in the tiles a plain group never writes (the slab sums read them for the up to three plain slabs behind q_gp),
    // and packed slabs lie across such tiles: the one-launch solve clears the buffer first (a solve after limo_ba_batch_reset that
    // follows a warm re-solve - rare, and a fill of a few MB)
    bool spart_has_packed = false;
    bool pristine = true;  // the device state is the state of create / reset: what a recovered barrier timeout of the one-launch solve restores
    // ---- the parts
    LockStep lock{*this};
    ShardExchange shards{*this};
    StreamSolve stream{*this};
    OneLaunch one{*this};
    IterationLog log{*this};
    PoseCovariance cov{*this};
    KernelTimers timers{*this};

    limo_ba_batch() = default;
    limo_ba_batch(const limo_ba_batch&) = delete;
    ~limo_ba_batch() {
        // (the arrays of P that live in the context's pinned pack arena are not freed one by one - kba_pack.hpp:PackArena -, the arena
        // is free for the next batch from here on; whatever of this batch's upload is still in flight only feeds device blocks that
        // go back to the pool below and are rewritten, in stream order, by their next user)
        if (holds_pack_arena) ctx->pack_arena_busy = false;
        for (auto& a : allocs) ctx->pool_free(a.first, a.second);
        if (h_pin) ctx->host_free(h_pin, sizeof(PinnedWords));
        lock.release_pinned();
        stream.teardown();
        timers.destroy_events();
        lock.destroy_events();
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

    int upload() {
        std::memset(&bv, 0, sizeof(bv));
        // Every buffer of the batch view lives in ONE device block: [initialised buffers | zero-filled buffers].
        // Small batches (a single window) stage the initialised part in pinned host memory and upload it with one
        // copy; large ones copy buffer by buffer (no second host copy of hundreds of MB).  One memset for the rest.
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
        // the measurements at the pair's index, from the slot table and the observations that have just been uploaded (the same stream)
        if (!P.evaluate_only && P.pair_m.empty()) {
            const int64_t n_pair = (int64_t)P.lm_slot.size();
            hipLaunchKernelGGL(k_pair_fill, dim3((unsigned)((n_pair + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, bv, n_pair);
            HIP_TRY(ctx, hipGetLastError());
        }
        pv.assign(1, bv);
        if (shards.setup()) return LIMO_ERR_RUNTIME;
        if (dmalloc((void**)&d_plane_rep, sizeof(double) * P.SO)) return LIMO_ERR_RUNTIME;
        if (dmalloc((void**)&d_plane_dep, sizeof(double) * P.SO)) return LIMO_ERR_RUNTIME;
        HIP_TRY(ctx, ctx->host_alloc((void**)&h_pin, sizeof(PinnedWords)));
        HIP_TRY(ctx, hipHostGetDevicePointer((void**)&d_pin, h_pin, 0));
        bv.n_active_host = nullptr;
        if (lock.alloc()) return LIMO_ERR_RUNTIME;
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
            cam_plan = plan_cam_lanes(P, cam_occ, shards.n_shards == 1 && !pose_batch);
        }
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_trim_select, hipFuncAttributeMaxDynamicSharedMemorySize, plan.trim_bytes));
        if (lock.create_events()) return LIMO_ERR_RUNTIME;
        return timers.create_events();
    }

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
    void launch_check(const char* what) { note(hipGetLastError(), what); }

    // The constants of a solve with options `o`: make_consts plus what depends on the batch's sharding alone (fixed at creation).
    // Schur granularity: a wave takes two plain Schur blocks (128 landmarks, 8 tiles) or one ground-plane block.  Fixed
    // (not a function of how many windows are in flight): the partial-slab layout of a window, and with it the order in
    // which its Schur complement is summed, is then the same alone and inside any batch - single-window and batched
    // solves give the same bits.  (Measured at 1024 C2 windows: span 2 is as fast as 4, span 1 costs 2 %.)
    // The spans also decide which slabs of S_part are "plain" (written in part only, kba_kernels.hip:schur_lean_group) - a slab must keep
    // its class for the life of the batch.
    SolveConsts consts_for(const limo_ba_options& o) const {
        SolveConsts k = make_consts(o);
        const bool sharded = shards.n_shards > 1;
        k.schur_span = sharded ? 1 : kSchurSpan;  // (Schur blocks are cut at shard boundaries)
        k.schur_span_gp = kSchurSpanGp;
        k.schur_nslab = sharded ? shards.n_shards : 0;
        k.schur_packed = sharded ? 1 : 0;
        // the launch sequences of an unsharded batch (lock-step and streaming) keep the partial slabs of fast-class windows packed
        // (kba_items.hpp:slab_packed_write); a sharded solve reduces tile slabs (slab_reduce_entry), and the one-launch solve, whose
        // own slab sum indexes the tile layout, gets a copy of the constants without it (solve_coop)
        k.slab_packed = sharded ? 0 : 1;
        return k;
    }

    // The options of a solve that differ from those of the last one.  min_landmarks_for_trimming decided do_trim at pack time: the
    // descriptors follow.  (Unsharded only: the one creator of a sharded batch, limo_ba_solve_sharded, solves with the options it created with.)
    int refresh_options(const limo_ba_options& o) {
        if (o.min_landmarks_for_trimming != opts.min_landmarks_for_trimming) {
            for (int w = 0; w < P.n_win; ++w) P.win[w].do_trim = P.win[w].n_lm > o.min_landmarks_for_trimming;
            HIP_TRY(ctx, hipMemcpyAsync((void*)bv.win, P.win.data(), sizeof(WinDesc) * P.n_win, hipMemcpyHostToDevice, ctx->stream));
        }
        opts = o;
        c = consts_for(o);
        return LIMO_OK;
    }

    // The per-window table of the solve that follows, in every view a kernel of it can be handed (unsharded: pv = {bv}; the slot
    // groups keep copies of bv).  null: a uniform solve - no kernel reads a record.
    void set_window_table(const WinOpts* t) {
        bv.wopt = t;
        for (BatchView& v : pv) v.wopt = t;
        for (StreamGroup& g : stream.groups) g.sv.wopt = t;
    }
    // wopt_host -> the device (the context's stream, in front of the solve's launches)
    int upload_window_table() {
        if (!d_wopt && dmalloc((void**)&d_wopt, sizeof(WinOpts) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
        HIP_TRY(ctx, hipMemcpyAsync(d_wopt, wopt_host.data(), sizeof(WinOpts) * wopt_host.size(), hipMemcpyHostToDevice, ctx->stream));
        set_window_table(d_wopt);
        return LIMO_OK;
    }

    // Which path this solve takes (kba_batch_plan.hpp:choose_solve_path, from run.sw and the context's strike counters).
    SolveChoice choose_path() {
        SolveFacts facts;
        facts.max_solver_time_sec = opts.max_solver_time_sec;
        facts.shard_P = shards.n_shards;
        facts.pose_batch = pose_batch;
        facts.pristine = pristine;
        facts.coop_strikes = ctx->coop_strikes;
        facts.coop_benched = ctx->coop_benched;
        const SolveChoice ch = choose_solve_path(P, plan, run.sw, facts);
        if (ch.benched) ++ctx->coop_benched;
        return ch;
    }
    // The launch sequence: slots (StreamSolve) or lock step (LockStep under run_schedule).
    void launch_sequence(SolvePath path) {
        run.path = path;
        if (path == PATH_STREAMING)
            stream.solve();
        else
            run_schedule(lock, opts);
    }
    void run_path(const SolveChoice& ch) {
        switch (ch.path) {
            case PATH_WG:
                run.path = PATH_WG;
                one.solve_wg();
                break;
            case PATH_COOP:
                if (one.solve_coop(ch.coop)) {
                    run.path = PATH_COOP;
                    run.coop_G = ch.coop.G;
                    ctx->coop_benched = 0;
                    break;
                }
                [[fallthrough]];  // the launch was refused (nothing ran)
            default:
                launch_sequence(ch.fallback);
        }
        pristine = false;
    }

    // The record of the solve into the context, for limo_ctx_last_solve_info / _schur_gp_info / _cam_lanes_info (limo_hip.h).
    void publish_run() {
        const bool streamed = run.path == PATH_STREAMING;
        long long* si = ctx->last_solve_info;
        si[0] = run.path;                                      // SolvePath
        si[1] = run.coop_redone ? 1 : 0;                       // a cooperative launch timed out and the solve was redone
        si[2] = run.coop_G;                                    // workgroups per window of the cooperative launch
        si[3] = streamed ? (long long)stream.groups.size() : 0;  // slot groups ...
        si[4] = streamed ? stream.n_slots : 0;                 // ... and slots of the streaming solve
        si[5] = run.n_rounds;                                  // its rounds
        si[6] = run.n_pair_launches;                           // launches of k_schur_lean_pair
        si[7] = run.lin_variant;                               // k_lin_lm<true> (1) / <false> (0)
        long long* gi = ctx->last_schur_gp_info;
        gi[0] = P.n_sgrp_narrow;          // narrow / three-panel ground-plane groups of the batch
        gi[1] = P.n_sgrp_wide;
        gi[2] = run.n_narrow_launches;    // launches that ran narrow / three-panel waves
        gi[3] = run.n_widegp_launches;
        long long* ci = ctx->last_cam_lanes_info;
        ci[0] = run.n_cam_launches[0][0];  // k_cam_assemble: half, full
        ci[1] = run.n_cam_launches[0][1];
        ci[2] = run.n_cam_launches[1][0];  // k_cam_solve: half, full
        ci[3] = run.n_cam_launches[1][1];
        ci[4] = cam_occ.asm_half;          // workgroups per CU of the four instances
        ci[5] = cam_occ.asm_full;
        ci[6] = cam_occ.solve_half;
        ci[7] = cam_occ.solve_full;
        ci[8] = 0;                         // windows whose camera system works in global memory
        for (const WinDesc& d : P.win) ci[8] += d.cam_scr_off >= 0 ? 1 : 0;
    }

    // k_lin_lm<true> (the default since round 6): four waves per SIMD, the window's view constants, the landmark block's running sums and
    // the tail's inputs in LDS (kba_kernels.hip:lin_lm_block) - scalar loads of the view constants return out of order, so every use of
    // one waited for all of them (round 5: 550 -> 513 us per round of 4096 slots through LDS).  With the camera-side sums in their raw
    // form (kba_items.hpp:lin_cam_half0: the 3 x 6 pose Jacobian is never formed) the kernel needs 129 registers instead of 149, so the
    // fourth wave costs nothing else: 505 -> 495 us per round, bench line +0.7 % against three waves.
    // Batches whose windows have so many views that the copy would cost occupancy (> 48 KB of LDS per workgroup: more than ~16 views)
    // and KBA_LIN_VLDS=0 (read once; the tests) take <false>: scalar loads - same bits in both variants.
    void launch_lin_lm(int grid, hipStream_t s, const BatchView& v, const int32_t* wl) {
        static const int want_vlds = std::getenv("KBA_LIN_VLDS") ? std::atoi(std::getenv("KBA_LIN_VLDS")) : 1;
        const bool vlds = want_vlds != 0 && lin_lm_lds_bytes(P.Vmax, true) <= 48 * 1024;
        const void* fn = vlds ? (const void*)k_lin_lm<true> : (const void*)k_lin_lm<false>;
        const int lds = lin_lm_lds_bytes(P.Vmax, vlds);
        run.lin_variant = vlds ? 1 : 0;
        if (lds > 48 * 1024 && lin_lds_set < lds) {  // (beyond the default dynamic-LDS limit: many views)
            note(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds), "hipFuncSetAttribute(k_lin_lm)");
            lin_lds_set = lds;
        }
        const BatchView* vp = &v;
        const SolveConsts* cp = &c;
        void* args[] = {(void*)vp, (void*)cp, (void*)&wl};
        note(hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, lds, s), "launch k_lin_lm");
    }

    // The Schur kernels of one view over its three lists, in this order: both fast-class lists in ONE launch where the caller allows
    // the pair kernel (kba_kernels.hip:k_schur_lean_pair), else plain groups, then ground-plane groups; then the generic windows.
    // Ground-plane groups of a batch in which the pack found narrow ones (plan.narrow; SchurGroup::gp_class), where the records' spans
    // and packed slabs are in use: k_schur_lean_gp, and k_schur_lean_pair<2, 3, true> in a draining round - their waves run the
    // narrow tile or the three-panel tile as the record says.  KBA_SCHUR_GP_WIDE: the three-panel kernels, as in every other batch.
    void launch_schur(const BatchView& v, const int32_t* wl_plain, int n_plain, const int32_t* wl_fgp, int n_fgp, const int32_t* wl_gen, int n_gen, bool pair,
                      hipStream_t s) {
        int span = c.schur_span, span_gp = c.schur_span_gp, packed = c.slab_packed;
        const bool narrow = plan.narrow && !run.sw.gp_wide && packed && span == kSchurSpan && span_gp == kSchurSpanGp;
        const bool wide = !narrow || P.n_sgrp_wide > 0;  // three-panel waves run
        if (pair) {
            void* args[] = {(void*)&v, (void*)&wl_plain, (void*)&n_plain, (void*)&wl_fgp, (void*)&span, (void*)&span_gp, (void*)&packed};
            note(hipLaunchKernel(narrow ? (const void*)k_schur_lean_pair<2, 3, true> : (const void*)k_schur_lean_pair<2, 3>, dim3(n_plain + n_fgp), dim3(64), args,
                                 std::max(plan.plain_lds, plan.leangp_lds), s),
                 "launch k_schur_lean_pair");
            ++run.n_pair_launches;
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
            run.n_narrow_launches += narrow ? 1 : 0;
            run.n_widegp_launches += wide ? 1 : 0;
        }
        if (n_gen) {
            void* args[] = {(void*)&v, (void*)&wl_gen, (void*)&span, (void*)&span_gp};
            note(hipLaunchKernel(schur_fn_gen, dim3(n_gen), dim3(64 * kWideWaves), args, plan.wide_lds, s), "launch k_schur_wide");
        }
    }

    // ---- the other kernels of the train, ONE launch site each: block size, dynamic LDS and argument order are fixed here; view,
    // worklist, grid and stream are the caller's - the lock-step solve (LockStep::linearize / assemble / step / trim) and the rounds of
    // the streaming solve (StreamSolve::enqueue_round).  A grid of 0 launches nothing.
    void launch_cam_assemble(const BatchView& v, const int32_t* list, int grid, hipStream_t s) {
        if (!grid) return;
        // (grid: the windows the launch can list - the same bits from either form, so the form is this launch's own choice)
        const bool half = cam_lanes_for_launch(cam_plan.asm_half_ok, cam_plan.asm_resident, grid, run.sw.cam_lanes) == kCamLanesHalf;
        if (half)
            hipLaunchKernelGGL(k_cam_assemble<kCamLanesHalf>, dim3(grid), dim3(kCamLanesHalf), plan.asm_bytes, s, v, c, list);
        else
            hipLaunchKernelGGL(k_cam_assemble<kBlock>, dim3(grid), dim3(kBlock), plan.asm_bytes, s, v, c, list);
        ++run.n_cam_launches[0][half ? 0 : 1];
    }
    void launch_cam_solve(const BatchView& v, const int32_t* list, int grid, hipStream_t s) {
        if (!grid) return;
        const bool half = cam_lanes_for_launch(cam_plan.solve_half_ok, cam_plan.solve_resident, grid, run.sw.cam_lanes) == kCamLanesHalf;
        if (half)
            hipLaunchKernelGGL(k_cam_solve<kCamLanesHalf>, dim3(grid), dim3(kCamLanesHalf), plan.solve_bytes, s, v, c, list);
        else
            hipLaunchKernelGGL(k_cam_solve<kBlock>, dim3(grid), dim3(kBlock), plan.solve_bytes, s, v, c, list);
        ++run.n_cam_launches[1][half ? 0 : 1];
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
        if (grid) hipLaunchKernelGGL(k_trim_max, dim3(grid), dim3(kBlock), 0, s, v, (const double*)d_plane_rep, (const double*)d_plane_dep, shard, shards.n_shards);
    }
    void launch_trim_select(const BatchView& v, int grid, hipStream_t s) {
        if (grid) hipLaunchKernelGGL(k_trim_select, dim3(grid), dim3(kBlock), plan.trim_bytes, s, v, c);
    }

    // An evaluation of an evaluate-only batch: the per-view constants + the materialised pass, on the context's stream.
    void launch_evaluate(int apply_loss, double* d_cost, uint8_t* d_valid) {
        hipLaunchKernelGGL(k_view_consts_all, dim3(cdiv(P.TV, 256)), dim3(256), 0, ctx->stream, bv);
        hipLaunchKernelGGL(k_evaluate, dim3(evaluate_grid(P.n_echunk)), dim3(kBlock), 0, ctx->stream, bv, c, apply_loss, d_cost, d_valid);
    }
};

// =============================================================================================== IterationLog
inline int IterationLog::bind(bool on) {
    limo_ctx* ctx = b.ctx;
    const int cap = on ? bound(b.opts) : 0;
    if (!on && !log_cap) return LIMO_OK;  // (never bound, or unbound already: the state holds no pointer)
    if (cap > log_alloc) {
        if (b.dmalloc((void**)&d_log, sizeof(limo_ba_iteration) * (size_t)cap * (size_t)std::max(1, b.P.n_win))) return LIMO_ERR_RUNTIME;
        log_alloc = cap;
    }
    if (cap != log_cap) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier reset may still read the image)
        for (int w = 0; w < b.P.n_win; ++w) {
            b.st0[w].log = on ? d_log + (size_t)w * cap : nullptr;
            b.st0[w].log_cap = cap;
        }
        log_cap = cap;
    }
    hipLaunchKernelGGL(k_log_bind, dim3(cdiv(b.P.n_win, 256)), dim3(256), 0, ctx->stream, b.bv, on ? d_log : (limo_ba_iteration*)nullptr, cap);
    HIP_TRY(ctx, hipGetLastError());
    return LIMO_OK;
}
// entries of window w -> host: *n = what the window has, at most `cap` written
inline int IterationLog::read(int w, int cap, limo_ba_iteration* out, int32_t* n) {
    limo_ctx* ctx = b.ctx;
    *n = 0;
    if (!log_cap) return LIMO_OK;
    WinState s;
    HIP_TRY(ctx, hipMemcpyAsync(&s, b.bv.st + w, sizeof(WinState), hipMemcpyDeviceToHost, ctx->stream));
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
inline int IterationLog::export_to_ctx() {
    limo_ctx* ctx = b.ctx;
    const PackedBatch& P = b.P;
    ctx->last_log.clear();
    ctx->last_log_n.clear();
    ctx->last_log_off.clear();
    if (!log_cap) return LIMO_OK;
    std::vector<WinState> sv(P.n_win);
    HIP_TRY(ctx, hipMemcpyAsync(sv.data(), b.bv.st, sizeof(WinState) * sv.size(), hipMemcpyDeviceToHost, ctx->stream));
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

// =============================================================================================== PoseCovariance
inline int PoseCovariance::ensure() {
    if (ready) return LIMO_OK;
    limo_ctx* ctx = b.ctx;
    const PackedBatch& P = b.P;
    cov_off.assign(P.n_win + 1, 0);
    std::vector<int64_t> scr_off(std::max(1, P.n_win), -1);
    int64_t scr_total = 0;
    lds_bytes = 0;
    for (int w = 0; w < P.n_win; ++w) {
        const WinDesc& d = P.win[w];
        cov_off[w + 1] = cov_off[w] + (int64_t)36 * d.n_kf * d.n_kf;
        const int doubles = cam_cov_scratch(d.nf, d.nfq), bytes = doubles * (int)sizeof(double);
        if (bytes > kCamLdsCapBytes) {
            scr_off[w] = scr_total;
            scr_total += doubles;
        } else {
            lds_bytes = std::max(lds_bytes, bytes);
        }
    }
    if (b.dmalloc((void**)&d_cov, sizeof(double) * (size_t)std::max<int64_t>(1, cov_off[P.n_win]))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_status, sizeof(int32_t) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_cov_off, sizeof(int64_t) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_scr_off, sizeof(int64_t) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_scratch, sizeof(double) * (size_t)std::max<int64_t>(1, scr_total))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_st_save, sizeof(WinState) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
    if (b.dmalloc((void**)&d_red_save, sizeof(WinRed) * std::max(1, P.n_win))) return LIMO_ERR_RUNTIME;
    if (P.n_win) {  // (synchronous copies: the host vectors are this call's)
        HIP_TRY(ctx, hipMemcpy(d_cov_off, cov_off.data(), sizeof(int64_t) * P.n_win, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(d_scr_off, scr_off.data(), sizeof(int64_t) * P.n_win, hipMemcpyHostToDevice));
    }
    ready = true;
    return LIMO_OK;
}

// The pass, on the context's stream behind the solve's last launch.  Not offered for a landmark-sharded batch.
inline int PoseCovariance::run() {
    limo_ctx* ctx = b.ctx;
    const PackedBatch& P = b.P;
    hipStream_t s = ctx->stream;
    computed = false;
    if (b.shards.n_shards > 1 || !offered || !P.n_win) return LIMO_OK;
    if (ensure() != LIMO_OK) return LIMO_ERR_RUNTIME;
    {   // the kernel's dynamic LDS limit belongs to the process, not to the batch: only ever raised
        static std::atomic<int> lds_limit{0};
        if (lds_bytes > lds_limit.load()) {
            HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_cam_cov, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
            lds_limit.store(lds_bytes);
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_st_save, b.bv.st, sizeof(WinState) * P.n_win, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_red_save, b.bv.red, sizeof(WinRed) * P.n_win, hipMemcpyDeviceToDevice, s));
    const SolveConsts keep = b.c;
    b.c.min_lm_diagonal = 0.0;  // clamp(a, 0, 0) = 0: lm_damp_store adds an exact zero for any finite radius
    b.c.max_lm_diagonal = 0.0;
    b.c.gradient_tolerance = -1.0;  // the decision behind the linearisation (lm_decide_lin) keeps every window active for the Schur waves
    b.c.min_radius = -1.0;
    b.lock.full_lists();
    const WorkLists& l = b.lock.wl[0].cur;
    hipLaunchKernelGGL(k_cov_begin, dim3(cdiv(P.n_win, 256)), dim3(256), 0, s, b.bv);
    b.launch_check("k_cov_begin");
    if (P.TV) {
        hipLaunchKernelGGL(k_view_consts, dim3(cdiv(P.TV, 256)), dim3(256), 0, s, b.bv);
        b.launch_check("k_view_consts");
    }
    if (l.n_lblk) {
        b.launch_lin_lm(l.n_lblk, s, b.bv, l.lblk);
        b.launch_check("k_lin_lm");
    }
    {
        BatchView bvs = b.bv;  // (the words of LockStep::assemble's slot 0: the next solve writes them before it reads them)
        bvs.n_active_host = b.d_pin->active;
        b.launch_cam_assemble(bvs, l.win, l.n_win, s);
        b.launch_check("k_cam_assemble");
    }
    if (l.n_sblk) {
        if (b.c.slab_packed) b.spart_has_packed = true;
        b.launch_schur(b.bv, l.sblk, l.n_sblk_plain, l.sblk + l.n_sblk_plain, l.n_sblk_fgp, l.sblk + l.n_sblk_plain + l.n_sblk_fgp,
                       l.n_sblk - l.n_sblk_plain - l.n_sblk_fgp, false, s);
        b.launch_check("Schur kernels");
    }
    hipLaunchKernelGGL(k_cam_cov, dim3(P.n_win), dim3(kBlock), lds_bytes, s, b.bv, b.c, d_cov, (const int64_t*)d_cov_off, (const int64_t*)d_scr_off, d_scratch, d_status);
    b.launch_check("k_cam_cov");
    b.c = keep;
    HIP_TRY(ctx, hipMemcpyAsync(b.bv.st, d_st_save, sizeof(WinState) * P.n_win, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(b.bv.red, d_red_save, sizeof(WinRed) * P.n_win, hipMemcpyDeviceToDevice, s));
    computed = b.rc == LIMO_OK;
    return b.rc;
}
// matrix and status of window w -> host
inline int PoseCovariance::read(int w, int64_t cap, double* out, int32_t* status) {
    limo_ctx* ctx = b.ctx;
    *status = LIMO_COV_NOT_COMPUTED;
    if (!computed) return LIMO_OK;
    const int64_t n = cov_off[w + 1] - cov_off[w];
    HIP_TRY(ctx, hipMemcpyAsync(status, d_status + w, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out && n) HIP_TRY(ctx, hipMemcpyAsync(out, d_cov + cov_off[w], sizeof(double) * (size_t)std::min(n, cap), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return LIMO_OK;
}
// every window's matrix into the context's buffer (limo_ctx_last_pose_covariance), for the calls that destroy their batch
inline int PoseCovariance::export_to_ctx() {
    limo_ctx* ctx = b.ctx;
    ctx->last_cov.clear();
    ctx->last_cov_status.clear();
    ctx->last_cov_off.clear();
    if (!computed) return LIMO_OK;
    const int n_win = b.P.n_win;
    ctx->last_cov.resize((size_t)cov_off[n_win]);
    ctx->last_cov_status.resize(n_win);
    ctx->last_cov_off.assign(cov_off.begin(), cov_off.end());
    if (cov_off[n_win]) HIP_TRY(ctx, hipMemcpyAsync(ctx->last_cov.data(), d_cov, sizeof(double) * (size_t)cov_off[n_win], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->last_cov_status.data(), d_status, sizeof(int32_t) * n_win, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return LIMO_OK;
}

// =============================================================================================== KernelTimers
inline int KernelTimers::create_events() {
    HIP_TRY(b.ctx, hipEventCreate(&ev_total_a));
    HIP_TRY(b.ctx, hipEventCreate(&ev_total_b));
    return LIMO_OK;
}
inline void KernelTimers::destroy_events() {
    for (auto& e : ev_pool) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    if (ev_total_a) (void)hipEventDestroy(ev_total_a);
    if (ev_total_b) (void)hipEventDestroy(ev_total_b);
}
// Event pair around one launch of a timed kernel (nullptr once the pool is exhausted); stop() records its end.
inline EventPair* KernelTimers::timed(int kernel, hipStream_t on) {
    if (ev_used >= 16384) return nullptr;
    if (ev_used == ev_pool.size()) {
        EventPair e;
        e.kernel = kernel;
        b.note(hipEventCreate(&e.a), "hipEventCreate");
        b.note(hipEventCreate(&e.b), "hipEventCreate");
        ev_pool.push_back(e);
    }
    EventPair* ep = &ev_pool[ev_used++];
    ep->kernel = kernel;
    b.note(hipEventRecord(ep->a, on ? on : b.ctx->stream), "hipEventRecord");
    return ep;
}
inline void KernelTimers::stop(EventPair* ep, hipStream_t s) {
    if (ep) b.note(hipEventRecord(ep->b, s), "hipEventRecord");
}
inline int KernelTimers::start_solve() {
    t0 = std::chrono::steady_clock::now();
    HIP_TRY(b.ctx, hipEventRecord(ev_total_a, b.ctx->stream));
    return LIMO_OK;
}
// (drains the context's stream: the solve is complete when this returns)
inline int KernelTimers::stop_solve() {
    limo_ctx* ctx = b.ctx;
    HIP_TRY(ctx, hipEventRecord(ev_total_b, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ev_total_a, ev_total_b));
    total_ms_acc += ms;
    last_solve_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return LIMO_OK;
}
inline int KernelTimers::collect() {
    if (ev_used) {
        HIP_TRY(b.ctx, hipStreamSynchronize(b.ctx->stream));
        for (size_t i = 0; i < ev_used; ++i) {
            float ms = 0.f;
            HIP_TRY(b.ctx, hipEventElapsedTime(&ms, ev_pool[i].a, ev_pool[i].b));
            k_ms_acc[ev_pool[i].kernel] += ms;
            k_launches[ev_pool[i].kernel] += 1;
        }
        ev_used = 0;
    }
    return LIMO_OK;
}

#include "limo_batch_lockstep.hpp"
#include "limo_batch_onelaunch.hpp"
#include "limo_batch_stream.hpp"
