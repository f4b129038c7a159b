// kba_batch_plan.hpp — what the host decides from a batch's packed layout.  ONCE per batch: which Schur kernel variants serve it and
// how much dynamic LDS every kernel of the solve gets (BatchPlan), and the Schur worklists (build_sblk_list).  Once per SOLVE: which
// launch path it takes (choose_solve_path, from the KBA_* switches of SolveSwitches) and the slot geometry of a streaming solve
// (stream_geometry).  Host-only and free of the HIP runtime, so that the decisions are testable without a device
// (tests/cpp/test_batch_plan.cpp); limo_batch.hpp turns the integers into kernel pointers and launches.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "kba_items.hpp"
#include "kba_pack.hpp"

namespace kba {

// What the plan needs from next to the kernels (kba_kernels.hip): their LDS-size helpers and two of their constants.
struct PlanKernelSizes {
    int (*lean_lds)(int ncol);                      // schur_lean_lds_bytes
    int (*wide_lds)(int nfp, int nc, int n_view);   // schur_wide_lds_bytes
    int lin_lds;                                    // lin_lm_lds_bytes(P.Vmax, true)
    int wide_waves;                                 // kWideWaves
    int trim_max_sort;                              // kTrimMaxSort
};

struct BatchPlan {
    bool any_fast = false, any_gen = false;
    // k_schur_lean<TM, false, WPE> of the plain groups and k_schur_lean<TM, true, WPE> of the ground-plane groups of fast-class windows;
    // the TMs are also the template arguments of the one-launch solve (k_solve_coop)
    int plain_tm = 1, plain_wpe = 4, gp_tm = 1, gp_wpe = 3;
    bool pair_ok = false;  // the variants are <2, false> / <3, true>: k_schur_lean_pair<2, 3> exists for them
    int wide_npw = 0;      // k_schur_wide<NPW> of the windows outside the fast class (chosen per batch maximum: results do not depend on
                           // what else is in the batch); 0: no such window; -1: a window with too many free camera slots
    int plain_lds = 0, leangp_lds = 0, wide_lds = 0;  // dynamic LDS bytes of the three
    int max_nc = 0;
    int asm_bytes = 0, solve_bytes = 0, trim_bytes = 0;  // k_cam_assemble, k_cam_solve, k_trim_select
    int schur_wave_lds = 0;  // LDS of one Schur wave inside the one-launch solve
    int onelaunch_lds = 0;   // the window-level phases of a one-launch solve (k_solve_wg; k_solve_coop adds its Schur waves)
    // gp_tm == 3 and the pack found narrow ground-plane groups (PackedBatch::n_sgrp_narrow): k_schur_lean_gp serves the ground-plane
    // groups - a narrow one on a tile of the pose columns, the rhs and one keyframe's <= 4 plane slots (two panels)
    bool narrow = false;
};

inline BatchPlan plan_batch(const PackedBatch& P, const PlanKernelSizes& ks) {
    BatchPlan p;
    int t_gen = 1, nfp_gen = 16, nc_gen = kCamSlots, nv_gen = 1, max_nfq = 0, max_nf = 0;
    for (const WinDesc& d : P.win) {
        p.max_nc = std::max(p.max_nc, (int)d.nc);
        if (d.schur_fast) {  // decided at pack time (kba_pack.cpp)
            p.any_fast = true;
            max_nfq = std::max(max_nfq, (int)d.nfq);
            max_nf = std::max(max_nf, (int)d.nf);
        } else if (d.n_sblk > 0) {
            p.any_gen = true;
            t_gen = std::max(t_gen, d.nf_pad / 16);
            nfp_gen = std::max(nfp_gen, (int)d.nf_pad);
            nc_gen = std::max(nc_gen, (int)d.nc);
            nv_gen = std::max(nv_gen, (int)d.n_view);
        }
    }
    if (p.any_fast) {
        p.plain_tm = (max_nfq + 16) / 16 <= 1 ? 1 : 2;
        p.plain_wpe = p.plain_tm == 1 ? 4 : 3;
        p.plain_lds = ks.lean_lds(max_nfq + 1);
        p.gp_tm = std::min(3, (max_nf + 16) / 16);
        p.gp_wpe = p.gp_tm == 1 ? 3 : 2;
        p.leangp_lds = ks.lean_lds(max_nf + 1);
        p.pair_ok = p.plain_tm == 2 && p.gp_tm == 3;
        p.narrow = p.gp_tm == 3 && P.n_sgrp_narrow > 0;
    }
    if (p.any_gen) {
        const int tiles = t_gen * (t_gen + 1) / 2, npw = (tiles + ks.wide_waves - 1) / ks.wide_waves;
        p.wide_npw = npw <= 1 ? 1 : npw <= 3 ? 3 : npw <= 6 ? 6 : npw <= 12 ? 12 : -1;
        p.wide_lds = ks.wide_lds(nfp_gen, nc_gen, nv_gen);
    }
    {   // LDS of the window-level kernels: the largest window that still works in LDS (the others: cam_scr_off)
        int nc_lds = kCamSlots, nf_lds = 1, nv_lds = 1;
        for (const WinDesc& d : P.win)
            if (d.cam_scr_off < 0) {
                nc_lds = std::max(nc_lds, (int)d.nc);
                nf_lds = std::max(nf_lds, (int)d.nf);
                nv_lds = std::max(nv_lds, (int)d.n_view);
            }
        p.asm_bytes = cam_assemble_scratch(nc_lds, kBlock, nv_lds) * (int)sizeof(double);
        p.solve_bytes = cam_solve_scratch(nc_lds, kBlock, nf_lds) * (int)sizeof(double);  // the compact system: nf <= nc free slots
    }
    int max_lm = 1, np2 = 1;
    for (const WinDesc& d : P.win) max_lm = std::max(max_lm, (int)d.n_lm);
    while (np2 < max_lm) np2 <<= 1;
    p.trim_bytes = np2 <= ks.trim_max_sort ? np2 * 12 + max_lm + 16 : 16;
    p.schur_wave_lds = (std::max(p.plain_lds, p.leangp_lds) + 15) / 16 * 16;
    p.onelaunch_lds = std::max(std::max(p.asm_bytes, p.solve_bytes), std::max(p.trim_bytes, ks.lin_lds));
    return p;
}

// Schur worklist over `windows` (all of them when null): first block of every group of `span` blocks of one class,
// ordered [plain groups of fast windows | ground-plane groups of fast windows | groups of generic windows];
// owner >= 0 keeps the blocks of that shard only.
inline void build_sblk_list(const PackedBatch& P, const std::vector<int32_t>* windows, int span, int span_gp, int owner, std::vector<int32_t>& v,
                            int& n_plain, int& n_fgp) {
    v.clear();
    n_plain = n_fgp = 0;
    const int nw = windows ? (int)windows->size() : P.n_win;
    for (int cls = 0; cls < 3; ++cls) {
        for (int q = 0; q < nw; ++q) {
            const int w = windows ? (*windows)[q] : q;
            const WinDesc& d = P.win[w];
            if ((cls < 2) != (d.schur_fast != 0)) continue;
            auto groups = [&](int i0, int i1, int sp) {
                for (int i = i0; i < i1; i += sp)
                    if (owner < 0 || P.sblk_owner[d.sblk0 + i] == owner) v.push_back(d.sblk0 + i);
            };
            if (cls != 1) groups(0, d.n_sblk_plain, span);
            if (cls != 0) groups(d.n_sblk_plain, d.n_sblk, span_gp);
        }
        if (cls == 0) n_plain = (int)v.size();
        if (cls == 1) n_fgp = (int)v.size() - n_plain;
    }
}

// ------------------------------------------------------------------------------------------------ the path of one solve
// At most 64 windows per cooperative launch (>= 4 workgroups per window): measured on C2 windows (scripts/gpu_small_batch.py), one
// launch vs streaming solve: 16 windows 10.8 / 19.1 ms, 64: 17.4 / 22.4 ms, 128: 25.0 / 24.0 ms, 256: 34.0 / 27.7 ms.
constexpr int kCoopMaxWg = 256, kCoopMaxWin = 64;
constexpr int kWgMaxLblk = 8;        // k_solve_wg: <= 2048 landmarks per window
constexpr int kCoopRetryAfter = 64;  // solves through the launch sequence before a benched cooperative path is tried again

// The KBA_* switches that steer a solve, read from the environment once per limo_ba_batch_solve (the tests switch paths between two
// solves of one process).  atoi; "0" means off.
struct SolveSwitches {
    bool stream_min_set = false;  // KBA_STREAM_MIN is set: the caller asks for the streaming solve wherever the batch can stream
    int stream_min = 16;          // ... windows from which a batch streams through slots
    int coop_max_win = kCoopMaxWin;  // KBA_COOP_MAX_WIN (timing aid, up to kCoopMaxWg): windows up to which a batch is one cooperative launch
    bool no_wg = false;           // KBA_NO_WG_SOLVE: never k_solve_wg
    bool no_coop = false;         // KBA_NO_COOP_SOLVE: never k_solve_coop
    double coop_timeout_ms = 50.0;  // KBA_COOP_TIMEOUT_MS: what a barrier of k_solve_coop waits before it gives the launch up
    bool groups_set = false;      // KBA_GROUPS is set ...
    int groups = 0;               // ... slot groups of a streaming solve (stream_geometry clamps to 1 .. 4) instead of its own rule
    int cam_lanes = 0;            // KBA_CAM_LANES (test hook): 128 / 256 force that form of the camera kernels where the batch allows it; else 0: cam_lanes_for_launch's rule
    bool gp_wide = false;        // KBA_SCHUR_GP_WIDE (debugging aid): every ground-plane group runs the three-panel tile, the narrow kernel never
};

inline SolveSwitches read_solve_switches() {
    SolveSwitches s;
    auto on = [](const char* name) {
        const char* e = std::getenv(name);
        return e && std::atoi(e) != 0;
    };
    if (const char* e = std::getenv("KBA_STREAM_MIN")) {
        s.stream_min_set = true;
        s.stream_min = std::atoi(e);
    }
    if (const char* e = std::getenv("KBA_COOP_MAX_WIN")) s.coop_max_win = std::min(std::atoi(e), kCoopMaxWg);
    s.no_wg = on("KBA_NO_WG_SOLVE");
    s.no_coop = on("KBA_NO_COOP_SOLVE");
    if (const char* e = std::getenv("KBA_COOP_TIMEOUT_MS")) s.coop_timeout_ms = std::atof(e);
    if (const char* e = std::getenv("KBA_GROUPS")) {
        s.groups_set = true;
        s.groups = std::atoi(e);
    }
    if (const char* e = std::getenv("KBA_CAM_LANES")) {
        const int v = std::atoi(e);
        s.cam_lanes = v == kCamLanesHalf || v == kBlock ? v : 0;
    }
    s.gp_wide = on("KBA_SCHUR_GP_WIDE");
    return s;
}

// ------------------------------------------------------------------------------------------------ lanes of the camera kernels
// k_cam_assemble / k_cam_solve exist with kBlock lanes per window and with kCamLanesHalf lanes that give every window the SAME bits
// (kba_items.hpp:cam_assemble, virtual lanes), so the choice is free per launch.  Half the lanes hold half the registers for the
// length of a window's dependent chain: twice the windows per CU, each somewhat slower.  That pays where a launch is bound by its
// passes over the device (windows / resident windows), not by one chain.
struct CamOccupancy {  // from the HIP runtime (limo_batch.hpp:upload): workgroups per CU at the plan's LDS sizes, compute units of the device
    int n_cu = 0;
    int asm_full = 0, asm_half = 0, solve_full = 0, solve_half = 0;
};
struct CamLanesPlan {
    bool asm_half_ok = false, solve_half_ok = false;  // the batch allows the half form of the kernel
    int asm_resident = 0, solve_resident = 0;         // windows the FULL form holds resident on the device
};
// Per batch.  The half form serves LDS-class windows whose slots one lane each covers (cam_assemble's slots_once), in the launch-
// sequence paths of an unsharded solve batch (`plain`: not sharded, not a pose-only batch - those keep kBlock lanes), and only where
// it at least doubles the workgroups per CU.  (The pack's LDS / global classification -
// kba_items.hpp:cam_class_doubles - does not depend on the form: no window changes class.)
inline CamLanesPlan plan_cam_lanes(const PackedBatch& P, const CamOccupancy& occ, bool plain) {
    CamLanesPlan p;
    p.asm_resident = occ.n_cu * occ.asm_full;
    p.solve_resident = occ.n_cu * occ.solve_full;
    bool ok = plain && P.n_win > 0;
    for (const WinDesc& d : P.win) ok = ok && d.cam_scr_off < 0 && d.nc <= kCamLanesHalf;
    p.asm_half_ok = ok && occ.asm_full > 0 && occ.asm_half >= 2 * occ.asm_full;
    p.solve_half_ok = ok && occ.solve_full > 0 && occ.solve_half >= 2 * occ.solve_full;
    return p;
}
// Per launch: the half form when the launch lists more windows than kCamLanesFactor x what the full form holds resident.  Below
// that - a draining round, a batch of ~1000 windows or fewer, a single window - the launch is one pass, bound by one chain: kBlock
// lanes.  forced: SolveSwitches::cam_lanes.
constexpr int kCamLanesFactor = 1;
inline int cam_lanes_for_launch(bool half_ok, int resident_full, int n_listed, int forced) {
    if (!half_ok || forced == kBlock) return kBlock;
    if (forced == kCamLanesHalf) return kCamLanesHalf;
    return n_listed > kCamLanesFactor * resident_full ? kCamLanesHalf : kBlock;
}

enum SolvePath { PATH_NONE = 0, PATH_WG = 1, PATH_COOP = 2, PATH_STREAMING = 3, PATH_LOCKSTEP = 4 };  // (limo_ctx_last_solve_info)

// What choose_solve_path needs to know beyond the packed batch, its plan and the switches.
struct SolveFacts {
    double max_solver_time_sec = -1.0;  // the option: a wall-clock cap keeps a batch out of the slot scheduler
    int shard_P = 1;
    bool pose_batch = false;  // made by limo_ba_batch_create_pose_only
    bool pristine = true;     // the device state is the state of create / reset
    int coop_strikes = 0, coop_benched = 0;  // the context's: cooperative launches that timed out in a row / solves benched since
};
struct CoopGeometry {
    int G = 0, grid = 0;  // workgroups per window; grid = 8 G ceil(n_win / 8), of which n_win G workgroups work (k_solve_coop)
};
struct SolveChoice {
    SolvePath path = PATH_LOCKSTEP;
    SolvePath fallback = PATH_LOCKSTEP;  // the launch sequence: what a refused or timed-out cooperative launch is redone with
    bool benched = false;  // three strikes keep this solve off the cooperative path: the caller counts it (coop_benched)
    CoopGeometry coop;     // path == PATH_COOP
};

// Schur groups (one per wave) of a window with `span` plain / `span_gp` ground-plane blocks per group
inline int plain_groups(const WinDesc& d, int span) { return (d.n_sblk_plain + span - 1) / span; }
inline int gp_groups(const WinDesc& d, int span_gp) { return (d.n_sblk - d.n_sblk_plain + span_gp - 1) / span_gp; }

// k_solve_wg (a whole solve in ONE launch, a workgroup per window): batches without a Schur block - adjustPoseOnly windows, and solve
// windows of any number of keyframes whose landmarks are all constant (PackOptions::lm_fixed) - whose landmark workgroups a single
// workgroup walks through in a few microseconds.
inline bool wg_solve_applies(const PackedBatch& P, const BatchPlan& plan, const SolveSwitches& sw, int shard_P) {
    if (shard_P != 1 || P.evaluate_only || P.n_sblk != 0 || P.n_win < 1 || sw.no_wg) return false;
    for (const WinDesc& d : P.win)
        if (d.n_lblk > kWgMaxLblk) return false;
    return plan.onelaunch_lds <= kCamLdsCapBytes;
}

inline int coop_lds_bytes(const BatchPlan& plan) { return std::max(plan.onelaunch_lds, (kBlock / 64) * plan.schur_wave_lds); }

// k_solve_coop (one window or a few, ONE launch): G workgroups per window that meet at device-wide barriers where the lock-step
// solve has launch boundaries.  Fast-class windows with their camera system in LDS only; an unsharded batch (spans kSchurSpan /
// kSchurSpanGp).
inline bool coop_solve_applies(const PackedBatch& P, const BatchPlan& plan, const SolveSwitches& sw, int shard_P, CoopGeometry& geo) {
    if (shard_P != 1 || P.evaluate_only || P.n_win < 1 || sw.no_coop) return false;
    int G = 1;
    for (const WinDesc& d : P.win) {
        if (!d.schur_fast || d.cam_scr_off >= 0 || d.nf_pad * d.nf_pad > kCoopRedStride) return false;
        const int tasks = plain_groups(d, kSchurSpan) + gp_groups(d, kSchurSpanGp);
        // enough workgroups for one landmark workgroup each, and for one Schur group per wave next to workgroup 0
        G = std::max(G, std::max((int)d.n_lblk, tasks ? 1 + (tasks + kBlock / 64 - 1) / (kBlock / 64) : 1));
    }
    G = std::min(G, 32);
    // one workgroup per CU, all resident: a batch of up to kCoopMaxWin windows shares the chip with fewer workgroups per
    // window (64 windows: 4 each) - still far ahead of ten launches per iteration over 64 slots
    if (P.n_win > kCoopMaxWg || coop_lds_bytes(plan) > kCamLdsCapBytes) return false;
    // the workgroups of a window on one XCD (k_solve_coop): 8 * per8 <= kCoopMaxWg follows from n_win <= kCoopMaxWg
    const int per8 = ((int)P.n_win + 7) / 8;
    geo.G = std::max(1, std::min(G, kCoopMaxWg / (8 * per8)));
    geo.grid = 8 * geo.G * per8;
    return true;
}

// Which path a solve takes.  Windows of a batch converge after very different numbers of iterations: from a few windows on they
// stream through slots (k_sched) instead of advancing in lock-step - not sharded solves (exchange steps between the kernels) and
// not with a wall-clock cap (a per-solve clock, run_schedule keeps it).  Small batches (<= coop_max_win windows of the common shape)
// run as ONE launch: a workgroup per window (no free landmark) or G workgroups per window.  All paths give the same bits.
// A batch of SEVERAL adjustPoseOnly windows takes k_solve_wg at any size - its workgroups never wait for each other, so the grid
// need not be resident at once - or else the lock-step sequence.  Never the slot scheduler and never device-wide barriers over several
// such windows: no test holds those paths for a pose-only batch.  (Windows without Schur blocks as such are no obstacle to either: a
// solve batch with constant landmarks may hold them - every landmark of a window flagged - and takes the paths of any solve batch;
// their Schur list counts are zero, tests/test_gpu_fixed_landmarks.py.)
// The cooperative solve starts only from the pristine state - its timeout recovery restores THAT state, a warm re-solve would lose
// the first solve's result - and not in a context whose launches keep timing out (something shares the GPU): three strikes switch
// it off, but not for the life of the context: the kCoopRetryAfter-th benched solve makes ONE more attempt (a profiler session or
// a neighbour process that has gone away); its success clears the strikes.  Pure: the caller applies the counter updates.
inline SolveChoice choose_solve_path(const PackedBatch& P, const BatchPlan& plan, const SolveSwitches& sw, const SolveFacts& f) {
    SolveChoice ch;
    const bool pose_multi = f.pose_batch && P.n_win > 1;
    const bool can_stream = f.shard_P == 1 && f.max_solver_time_sec <= 0.0 && P.n_win >= sw.stream_min && !P.evaluate_only && !pose_multi;
    const bool one_launch = pose_multi || (!(sw.stream_min_set && can_stream) && P.n_win <= sw.coop_max_win);
    ch.path = ch.fallback = can_stream ? PATH_STREAMING : PATH_LOCKSTEP;
    if (!one_launch) return ch;
    if (wg_solve_applies(P, plan, sw, f.shard_P)) {
        ch.path = PATH_WG;
    } else if (!pose_multi && f.pristine && coop_solve_applies(P, plan, sw, f.shard_P, ch.coop)) {
        ch.benched = f.coop_strikes >= 3;
        if (!ch.benched || f.coop_benched + 1 >= kCoopRetryAfter) ch.path = PATH_COOP;
    }
    return ch;
}

// ------------------------------------------------------------------------------------------------ slots of a streaming solve
struct SchurSpans {
    int plain = kSchurSpan, gp = kSchurSpanGp;  // SolveConsts::schur_span / schur_span_gp
};
struct StreamGeometry {
    int n_slots = 0, n_groups = 0;
    int group_slots[4] = {0, 0, 0, 0};  // [n_groups], each <= kSchedMaxSlots
    int mx[SL_COUNT] = {0};             // entries of list k a single window can have
};
inline StreamGeometry stream_geometry(const PackedBatch& P, const SchurSpans& spans, const SolveSwitches& sw) {
    StreamGeometry g;
    // windows in flight: a quarter of the batch (so that the ramp-down at the end of the batch is a small part of the
    // solve), at least 1024 (a round of fewer windows is bound by the latency of its window-level kernels)
    g.n_slots = std::min((int)P.n_win, std::max(1024, std::min(kSchedMaxSlots, (int)P.n_win / 4)));
    // two slot groups from 512 windows on (A/B at 256 .. 1536 windows: 5-9 % on the re-solve at every size; the FIRST solve of a batch
    // pays the second group's streams and events, which a one-shot batch of 256 windows does not earn back: 44 vs 36 ms)
    // THREE groups once a group still holds ~1400 slots (4096 slots = batches of 16384 windows: 36.4 vs 35.8 k windows/s, alternating runs
    // on one box; at 1024-2048 slots a third group costs 1-4 %, a fourth 7 % at 4096: profiles/r06_experiment_launch_train.txt)
    g.n_groups = sw.groups_set ? std::max(1, std::min(4, sw.groups)) : g.n_slots >= 4096 ? 3 : P.n_win >= 512 ? 2 : 1;
    for (int gi = 0; gi < g.n_groups; ++gi) g.group_slots[gi] = g.n_slots / g.n_groups + (gi < g.n_slots % g.n_groups ? 1 : 0);
    for (const WinDesc& d : P.win) {
        const int plg = plain_groups(d, spans.plain), gpg = gp_groups(d, spans.gp);
        g.mx[SL_LBLK] = std::max(g.mx[SL_LBLK], (int)d.n_lblk);
        g.mx[SL_TBLK] = std::max(g.mx[SL_TBLK], (int)d.n_blk);
        g.mx[SL_SPLAIN] = std::max(g.mx[SL_SPLAIN], d.schur_fast ? plg : 0);
        g.mx[SL_SFGP] = std::max(g.mx[SL_SFGP], d.schur_fast ? gpg : 0);
        g.mx[SL_SGEN] = std::max(g.mx[SL_SGEN], d.schur_fast ? 0 : plg + gpg);
    }
    g.mx[SL_WIN] = 1;
    g.mx[SL_TLBLK] = g.mx[SL_LBLK];
    g.mx[SL_TWIN] = 1;
    return g;
}

}  // namespace kba
