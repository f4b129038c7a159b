// Host-only checks of limo_amd/csrc/kba_batch_plan.hpp (the per-batch kernel plan, the Schur worklist builder, the path of a solve
// and the slot geometry of the streaming solve) and of the pack arena's lend guard (kba_pack.hpp:PackArenaLend).  Stand-alone program, built with -fsanitize=address by tests/test_batch_plan_cpu.py
// together with kba_pack.cpp.  The expected values are written out here, not computed by the code under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../limo_amd/csrc/kba_batch_plan.hpp"

using namespace kba;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_failed;                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
        }                                                                  \
    } while (0)

// stand-ins for the LDS-size helpers next to the kernels: the plan has to call them with the right arguments
static int lean_lds(int ncol) { return 1000 + 8 * ncol; }
static int wide_lds(int nfp, int nc, int n_view) { return 100000 + 100 * nfp + 10 * nc + n_view; }
static const PlanKernelSizes kSizes = {lean_lds, wide_lds, /*lin_lds*/ 7000, /*wide_waves*/ 8, /*trim_max_sort*/ 8192};

static WinDesc window(int fast, int n_sblk_plain, int n_sblk) {
    WinDesc d;
    std::memset(&d, 0, sizeof(d));
    d.schur_fast = fast;
    d.n_sblk_plain = n_sblk_plain;
    d.n_sblk = n_sblk;
    d.n_kf = 3;
    d.nc = 30;
    d.nf = 20;
    d.nfq = 12;
    d.nf_pad = 32;
    d.n_view = 3;
    d.n_lm = 300;
    d.cam_scr_off = -1;
    return d;
}
static PackedBatch batch_of(const std::vector<WinDesc>& ws) {
    PackedBatch P;
    P.n_win = (int32_t)ws.size();
    P.win = ws;
    int sb = 0;
    for (WinDesc& d : P.win) {
        d.sblk0 = sb;
        sb += d.n_sblk;
    }
    P.n_sblk = sb;
    return P;
}

static void test_plan_table() {
    struct Row {
        int nfq, nf, plain_tm, plain_wpe, gp_tm, gp_wpe;
        bool pair;
    };
    const Row rows[] = {{0, 0, 1, 4, 1, 3, false},  {12, 20, 1, 4, 2, 2, false}, {15, 15, 1, 4, 1, 3, false},
                        {16, 16, 2, 3, 2, 2, false}, {18, 30, 2, 3, 2, 2, false}, {24, 40, 2, 3, 3, 2, true}};
    for (const Row& r : rows) {
        WinDesc d = window(1, 2, 3);
        d.nfq = r.nfq;
        d.nf = r.nf;
        const BatchPlan p = plan_batch(batch_of({d}), kSizes);
        CHECK(p.any_fast && !p.any_gen && p.wide_npw == 0);
        CHECK(p.plain_tm == r.plain_tm && p.plain_wpe == r.plain_wpe);
        CHECK(p.gp_tm == r.gp_tm && p.gp_wpe == r.gp_wpe);
        CHECK(p.pair_ok == r.pair);
        CHECK(p.plain_lds == 1000 + 8 * (r.nfq + 1) && p.leangp_lds == 1000 + 8 * (r.nf + 1));
        CHECK(p.schur_wave_lds == (1000 + 8 * (r.nf + 1) + 15) / 16 * 16);  // nf >= nfq: the ground-plane variant is the larger one
        CHECK(p.schur_wave_lds % 16 == 0 && p.schur_wave_lds >= p.plain_lds && p.schur_wave_lds >= p.leangp_lds && p.schur_wave_lds < p.leangp_lds + 16);
    }
    const int t_of[] = {1, 4, 5, 6, 7, 9, 10, 13, 14}, npw_of[] = {1, 3, 3, 3, 6, 6, 12, 12, -1};
    for (int k = 0; k < 9; ++k) {
        WinDesc d = window(0, 2, 3);
        d.nf_pad = 16 * t_of[k];
        d.nc = 70;
        d.n_view = 7;
        const BatchPlan p = plan_batch(batch_of({d}), kSizes);
        CHECK(!p.any_fast && p.any_gen && p.wide_npw == npw_of[k]);
        CHECK(p.wide_lds == 100000 + 100 * 16 * t_of[k] + 10 * 70 + 7);
        CHECK(p.plain_tm == 1 && p.gp_tm == 1 && !p.pair_ok && p.schur_wave_lds == 0);
    }
    {   // a generic window without Schur blocks does not count; the maxima run over the windows of each class
        WinDesc a = window(1, 2, 3), b = window(1, 1, 1), g0 = window(0, 0, 0), g1 = window(0, 1, 2);
        a.nfq = 24;
        a.nf = 30;
        b.nfq = 6;
        b.nf = 40;
        g0.nf_pad = 16 * 14;
        g1.nf_pad = 16 * 7;
        g1.nc = 70;
        b.n_lm = 9000;
        const BatchPlan p = plan_batch(batch_of({a, b, g0, g1}), kSizes);
        CHECK(p.plain_tm == 2 && p.gp_tm == 3 && p.pair_ok && p.wide_npw == 6);
        CHECK(p.plain_lds == 1000 + 8 * 25 && p.leangp_lds == 1000 + 8 * 41);
        CHECK(p.max_nc == 70);
        CHECK(p.trim_bytes == 16);  // 9000 landmarks: beyond the sort in LDS
        CHECK(p.asm_bytes == cam_assemble_scratch(70, kBlock, 3) * 8 && p.solve_bytes == cam_solve_scratch(70, kBlock, 40) * 8);
        int m = p.asm_bytes > p.solve_bytes ? p.asm_bytes : p.solve_bytes;
        CHECK(p.onelaunch_lds == (m > 7000 ? m : 7000));
    }
    {   // trimming sort: 300 landmarks -> 512 places
        const BatchPlan p = plan_batch(batch_of({window(1, 2, 3)}), kSizes);
        CHECK(p.trim_bytes == 512 * 12 + 300 + 16);
        CHECK(p.asm_bytes == cam_assemble_scratch(30, kBlock, 3) * 8 && p.solve_bytes == cam_solve_scratch(30, kBlock, 20) * 8);
    }
}

static void test_worklists() {
    PackedBatch P = batch_of({window(1, 5, 7), window(0, 3, 4), window(1, 0, 2), window(1, 4, 4)});  // sblk0 = 0, 7, 11, 13
    CHECK(P.n_sblk == 17);
    P.sblk_owner.resize(17);
    for (int k = 0; k < 17; ++k) P.sblk_owner[k] = k % 3;
    std::vector<int32_t> v;
    int n_plain = -1, n_fgp = -1;
    build_sblk_list(P, nullptr, 2, 1, -1, v, n_plain, n_fgp);
    CHECK((v == std::vector<int32_t>{0, 2, 4, 13, 15, 5, 6, 11, 12, 7, 9, 10}));
    CHECK(n_plain == 3 + 0 + 2 && n_fgp == 2 + 2 + 0);
    // span 1: the owners' lists partition the unfiltered list and keep its order
    std::vector<int32_t> u;
    int up = 0, ug = 0;
    build_sblk_list(P, nullptr, 1, 1, -1, u, up, ug);
    CHECK((u == std::vector<int32_t>{0, 1, 2, 3, 4, 13, 14, 15, 16, 5, 6, 11, 12, 7, 8, 9, 10}) && up == 9 && ug == 4);
    size_t total = 0;
    for (int owner = 0; owner < 3; ++owner) {
        build_sblk_list(P, nullptr, 1, 1, owner, v, n_plain, n_fgp);
        std::vector<int32_t> want;
        int wp = 0, wg = 0;
        for (size_t k = 0; k < u.size(); ++k)
            if (u[k] % 3 == owner) {
                want.push_back(u[k]);
                wp += k < 9;
                wg += k >= 9 && k < 13;
            }
        CHECK(v == want && n_plain == wp && n_fgp == wg);
        total += v.size();
    }
    CHECK(total == u.size());
    // a subset of the windows: the full list restricted to them
    const std::vector<int32_t> sub = {0, 3};
    build_sblk_list(P, &sub, 2, 1, -1, v, n_plain, n_fgp);
    CHECK((v == std::vector<int32_t>{0, 2, 4, 13, 15, 5, 6}) && n_plain == 5 && n_fgp == 2);
}

static void test_lend_guard() {
    char* block = static_cast<char*>(std::malloc(1u << 20));
    bool caught = false;
    try {
        PackArena arena;
        arena.base = block;
        arena.cap = 1u << 20;
        PackArenaLend loan(&arena);
        CHECK(pack_arena_take(128u << 10) == block);
        throw std::bad_alloc();
    } catch (const std::bad_alloc&) {
        caught = true;
    }
    CHECK(caught);
    CHECK(pack_arena_take(128u << 10) == nullptr);  // the loan ended with the scope: the arena object is gone
    {
        uvec<double> x(1 << 15);  // 256 KB, arena-sized: from the heap now
        x[0] = 1.0;
        x[(1 << 15) - 1] = 2.0;
        CHECK(!(reinterpret_cast<char*>(x.data()) >= block && reinterpret_cast<char*>(x.data()) < block + (1u << 20)));
    }
    std::free(block);
}

// ---- the path of a solve (choose_solve_path).  Expected values by hand from the rules: a batch streams from 16 windows on (not
// sharded, not capped, not several pose-only windows); up to 64 windows it is one launch instead unless KBA_STREAM_MIN is set and it
// can stream; k_solve_wg for windows without Schur blocks and <= 8 landmark workgroups, else k_solve_coop for fast-class windows
// from the pristine state.
static WinDesc fast_window(int n_lblk) {  // 5 plain + 2 ground-plane Schur blocks: 3 + 2 groups -> 1 + ceil(5 / 4) = 3 workgroups
    WinDesc d = window(1, 5, 7);
    d.n_lblk = n_lblk;
    d.n_blk = 4;
    return d;
}
static WinDesc pose_window(int n_lblk) {  // no free landmark: no Schur block
    WinDesc d = window(1, 0, 0);
    d.n_lblk = n_lblk;
    d.n_blk = 1;
    return d;
}
static SolveChoice choose(const std::vector<WinDesc>& ws, const SolveSwitches& sw, const SolveFacts& f, const PlanKernelSizes& ks = kSizes) {
    const PackedBatch P = batch_of(ws);
    return choose_solve_path(P, plan_batch(P, ks), sw, f);
}
static int lean_lds_huge(int) { return 40000; }  // four waves of it: 160000 > kCamLdsCapBytes

static void test_solve_paths() {
    const SolveSwitches def;
    const SolveFacts fresh;
    CHECK(def.stream_min == 16 && !def.stream_min_set && def.coop_max_win == 64 && !def.no_wg && !def.no_coop && def.coop_timeout_ms == 50.0 && !def.groups_set);
    CHECK(fresh.shard_P == 1 && fresh.pristine && !fresh.pose_batch && fresh.max_solver_time_sec <= 0.0 && fresh.coop_strikes == 0);
    SolveSwitches no_coop, no_wg, neither;
    no_coop.no_coop = neither.no_coop = true;
    no_wg.no_wg = neither.no_wg = true;
    {   // one fast window
        SolveChoice ch = choose({fast_window(2)}, def, fresh);
        CHECK(ch.path == PATH_COOP && ch.fallback == PATH_LOCKSTEP && !ch.benched);
        CHECK(ch.coop.G == 3 && ch.coop.grid == 24);  // the Schur groups ask for 3 workgroups
        ch = choose({fast_window(6)}, def, fresh);
        CHECK(ch.path == PATH_COOP && ch.coop.G == 6 && ch.coop.grid == 48);  // the landmark workgroups for 6
        ch = choose({fast_window(40)}, def, fresh);
        CHECK(ch.path == PATH_COOP && ch.coop.G == 32 && ch.coop.grid == 256);  // at most 32
        ch = choose({fast_window(2)}, no_coop, fresh);
        CHECK(ch.path == PATH_LOCKSTEP && ch.fallback == PATH_LOCKSTEP && !ch.benched);
        ch = choose({fast_window(2)}, no_wg, fresh);
        CHECK(ch.path == PATH_COOP);
    }
    {   // a window without Schur blocks
        SolveChoice ch = choose({pose_window(1)}, def, fresh);
        CHECK(ch.path == PATH_WG && ch.fallback == PATH_LOCKSTEP);
        ch = choose({pose_window(8)}, def, fresh);
        CHECK(ch.path == PATH_WG);
        ch = choose({pose_window(9)}, def, fresh);  // too many landmark workgroups for one workgroup to walk
        CHECK(ch.path == PATH_COOP && ch.coop.G == 9 && ch.coop.grid == 72);
        ch = choose({pose_window(1)}, no_wg, fresh);
        CHECK(ch.path == PATH_COOP && ch.coop.G == 1 && ch.coop.grid == 8);
        ch = choose({pose_window(1)}, no_coop, fresh);
        CHECK(ch.path == PATH_WG);
        ch = choose({pose_window(1)}, neither, fresh);
        CHECK(ch.path == PATH_LOCKSTEP);
    }
    {   // 24 fast windows
        const std::vector<WinDesc> ws(24, fast_window(2));
        SolveChoice ch = choose(ws, def, fresh);
        CHECK(ch.path == PATH_COOP && ch.fallback == PATH_STREAMING && ch.coop.G == 3 && ch.coop.grid == 72);
        SolveSwitches sm1, sm1000, sm1000_nc;
        sm1.stream_min_set = sm1000.stream_min_set = sm1000_nc.stream_min_set = true;
        sm1.stream_min = 1;
        sm1000.stream_min = sm1000_nc.stream_min = 1000;
        sm1000_nc.no_coop = true;
        ch = choose(ws, sm1, fresh);
        CHECK(ch.path == PATH_STREAMING && ch.fallback == PATH_STREAMING);
        ch = choose(ws, sm1000, fresh);
        CHECK(ch.path == PATH_COOP && ch.fallback == PATH_LOCKSTEP);
        ch = choose(ws, sm1000_nc, fresh);
        CHECK(ch.path == PATH_LOCKSTEP && ch.fallback == PATH_LOCKSTEP);
        ch = choose({fast_window(2)}, sm1, fresh);  // a single window streams when it is asked to
        CHECK(ch.path == PATH_STREAMING);
        std::vector<WinDesc> mixed = ws;
        mixed[7] = window(0, 3, 4);  // one generic-class window
        ch = choose(mixed, def, fresh);
        CHECK(ch.path == PATH_STREAMING && ch.fallback == PATH_STREAMING && !ch.benched);
        mixed[7] = fast_window(2);
        mixed[7].cam_scr_off = 0;  // camera system in global scratch
        CHECK(choose(mixed, def, fresh).path == PATH_STREAMING);
        mixed[7].cam_scr_off = -1;
        mixed[7].nf_pad = 80;  // 6400 > kCoopRedStride
        CHECK(choose(mixed, def, fresh).path == PATH_STREAMING);
        SolveFacts capped;
        capped.max_solver_time_sec = 5.0;
        ch = choose(ws, def, capped);
        CHECK(ch.path == PATH_COOP && ch.fallback == PATH_LOCKSTEP);
        ch = choose(ws, no_coop, capped);
        CHECK(ch.path == PATH_LOCKSTEP);
        CHECK(choose({fast_window(2)}, no_coop, capped).path == PATH_LOCKSTEP);
        SolveFacts warm;
        warm.pristine = false;
        CHECK(choose(ws, def, warm).path == PATH_STREAMING);
        CHECK(choose({fast_window(2)}, def, warm).path == PATH_LOCKSTEP);
        CHECK(choose({pose_window(1)}, def, warm).path == PATH_WG);  // (k_solve_wg has no barrier to time out: any state)
        SolveFacts sharded;
        sharded.shard_P = 2;
        CHECK(choose({fast_window(2)}, def, sharded).path == PATH_LOCKSTEP);
        CHECK(choose({pose_window(1)}, def, sharded).path == PATH_LOCKSTEP);
        CHECK(choose(ws, def, sharded).path == PATH_LOCKSTEP && choose(ws, def, sharded).fallback == PATH_LOCKSTEP);
    }
    {   // how many windows are one launch
        CHECK(choose(std::vector<WinDesc>(64, fast_window(2)), def, fresh).path == PATH_COOP);
        CHECK(choose(std::vector<WinDesc>(65, fast_window(2)), def, fresh).path == PATH_STREAMING);
        SolveSwitches wide;
        wide.coop_max_win = 256;
        SolveChoice ch = choose(std::vector<WinDesc>(200, fast_window(2)), wide, fresh);
        CHECK(ch.path == PATH_COOP && ch.fallback == PATH_STREAMING && ch.coop.G == 1 && ch.coop.grid == 200);
        CHECK(choose(std::vector<WinDesc>(257, fast_window(2)), wide, fresh).path == PATH_STREAMING);
        // cooperative grids: windows that ask for 32 workgroups each share 256
        const int n_of[] = {1, 40, 64, 200, 256}, g_of[] = {32, 6, 4, 1, 1}, grid_of[] = {256, 240, 256, 200, 256};
        for (int k = 0; k < 5; ++k) {
            ch = choose(std::vector<WinDesc>(n_of[k], fast_window(40)), wide, fresh);
            CHECK(ch.path == PATH_COOP && ch.coop.G == g_of[k] && ch.coop.grid == grid_of[k]);
            CHECK(ch.coop.grid <= 256 && ch.coop.grid == 8 * ch.coop.G * ((n_of[k] + 7) / 8));
        }
    }
    {   // three strikes bench the cooperative path; the 64th benched solve tries again
        SolveFacts f;
        f.coop_strikes = 2;
        SolveChoice ch = choose({fast_window(2)}, def, f);
        CHECK(ch.path == PATH_COOP && !ch.benched);
        f.coop_strikes = 3;
        const int benched_of[] = {0, 62, 63, 64};
        const SolvePath path_of[] = {PATH_LOCKSTEP, PATH_LOCKSTEP, PATH_COOP, PATH_COOP};
        for (int k = 0; k < 4; ++k) {
            f.coop_benched = benched_of[k];
            ch = choose({fast_window(2)}, def, f);
            CHECK(ch.path == path_of[k] && ch.benched && ch.fallback == PATH_LOCKSTEP);
        }
        f.coop_benched = 0;
        ch = choose(std::vector<WinDesc>(24, fast_window(2)), def, f);
        CHECK(ch.path == PATH_STREAMING && ch.benched);
        // a solve the cooperative path would not have taken anyway is not counted
        CHECK(!choose({fast_window(2)}, no_coop, f).benched);
        CHECK(!choose({pose_window(1)}, def, f).benched && choose({pose_window(1)}, def, f).path == PATH_WG);
        CHECK(!choose(std::vector<WinDesc>(65, fast_window(2)), def, f).benched);
        f.pristine = false;
        CHECK(!choose({fast_window(2)}, def, f).benched);
    }
    {   // several pose-only windows: k_solve_wg at any size, else lock-step
        SolveFacts pb;
        pb.pose_batch = true;
        std::vector<WinDesc> ws(300, pose_window(1));
        SolveChoice ch = choose(ws, def, pb);
        CHECK(ch.path == PATH_WG && ch.fallback == PATH_LOCKSTEP);
        ws[100].n_lblk = 9;
        SolveSwitches sm1;
        sm1.stream_min_set = true;
        sm1.stream_min = 1;
        ch = choose(ws, def, pb);
        CHECK(ch.path == PATH_LOCKSTEP && ch.fallback == PATH_LOCKSTEP && !ch.benched);
        ch = choose(ws, sm1, pb);
        CHECK(ch.path == PATH_LOCKSTEP && ch.fallback == PATH_LOCKSTEP);
        ws.resize(24);  // (24 windows without the large one)
        CHECK(choose(ws, no_wg, pb).path == PATH_LOCKSTEP);  // never barriers over several such windows
        CHECK(choose({pose_window(1)}, no_wg, pb).path == PATH_COOP);  // one window of a pose batch: as limo_ba_adjust_pose_only
    }
    {   // LDS beyond kCamLdsCapBytes refuses the one-launch kernels
        PlanKernelSizes big_lin = kSizes, big_wave = kSizes;
        big_lin.lin_lds = 200000;  // the window-level phases: both kernels
        big_wave.lean_lds = lean_lds_huge;  // the Schur waves: k_solve_coop only
        CHECK(choose({pose_window(1)}, def, fresh, big_lin).path == PATH_LOCKSTEP);
        CHECK(choose({fast_window(2)}, def, fresh, big_lin).path == PATH_LOCKSTEP);
        CHECK(choose(std::vector<WinDesc>(24, fast_window(2)), def, fresh, big_lin).path == PATH_STREAMING);
        CHECK(choose({pose_window(1)}, def, fresh, big_wave).path == PATH_WG);
        CHECK(choose({fast_window(2)}, def, fresh, big_wave).path == PATH_LOCKSTEP);
    }
}

static void test_stream_geometry() {
    const SolveSwitches def;
    const SchurSpans spans;
    CHECK(spans.plain == 2 && spans.gp == 1 && kSchedMaxSlots == 4096);
    struct Row {
        int n_win, slots, groups, per_group[4];
    };
    const Row rows[] = {{16, 16, 1, {16, 0, 0, 0}},          {512, 512, 2, {256, 256, 0, 0}},          {4096, 1024, 2, {512, 512, 0, 0}},
                        {8192, 2048, 2, {1024, 1024, 0, 0}}, {16384, 4096, 3, {1366, 1365, 1365, 0}}, {20000, 4096, 3, {1366, 1365, 1365, 0}},
                        {511, 511, 1, {511, 0, 0, 0}},       {1, 1, 1, {1, 0, 0, 0}},                  {5000, 1250, 2, {625, 625, 0, 0}}};
    for (const Row& r : rows) {
        const StreamGeometry g = stream_geometry(batch_of(std::vector<WinDesc>(r.n_win, fast_window(2))), spans, def);
        CHECK(g.n_slots == r.slots && g.n_groups == r.groups);
        for (int k = 0; k < 4; ++k) CHECK(g.group_slots[k] == r.per_group[k] && g.group_slots[k] <= kSchedMaxSlots);
    }
    {   // KBA_GROUPS: 1 .. 4
        SolveSwitches sw;
        sw.groups_set = true;
        const PackedBatch P = batch_of(std::vector<WinDesc>(512, fast_window(2)));
        sw.groups = 0;
        StreamGeometry g = stream_geometry(P, spans, sw);
        CHECK(g.n_groups == 1 && g.n_slots == 512 && g.group_slots[0] == 512 && g.group_slots[1] == 0);
        sw.groups = 9;
        g = stream_geometry(P, spans, sw);
        CHECK(g.n_groups == 4 && g.group_slots[0] == 128 && g.group_slots[1] == 128 && g.group_slots[2] == 128 && g.group_slots[3] == 128);
        sw.groups = 3;
        g = stream_geometry(P, spans, sw);
        CHECK(g.n_groups == 3 && g.group_slots[0] == 171 && g.group_slots[1] == 171 && g.group_slots[2] == 170 && g.group_slots[3] == 0);
        sw.groups = 1;
        g = stream_geometry(batch_of(std::vector<WinDesc>(20000, fast_window(2))), spans, sw);
        CHECK(g.n_groups == 1 && g.group_slots[0] == 4096 && g.group_slots[0] <= kSchedMaxSlots);
    }
    {   // entries a single window can have per list: a fast window (5 + 2 Schur blocks, 3 landmark and 4 observation workgroups) and a
        // generic one (3 + 1 blocks, 5 and 2)
        WinDesc gen = window(0, 3, 4);
        gen.n_lblk = 5;
        gen.n_blk = 2;
        const PackedBatch P = batch_of({fast_window(3), gen});
        StreamGeometry g = stream_geometry(P, spans, def);
        CHECK(g.n_slots == 2 && g.n_groups == 1);
        CHECK(g.mx[SL_LBLK] == 5 && g.mx[SL_TBLK] == 4 && g.mx[SL_TLBLK] == 5 && g.mx[SL_WIN] == 1 && g.mx[SL_TWIN] == 1);
        CHECK(g.mx[SL_SPLAIN] == 3 && g.mx[SL_SFGP] == 2 && g.mx[SL_SGEN] == 2 + 1);
        SchurSpans one;
        one.plain = 1;
        g = stream_geometry(P, one, def);
        CHECK(g.mx[SL_SPLAIN] == 5 && g.mx[SL_SFGP] == 2 && g.mx[SL_SGEN] == 3 + 1);
    }
}

static void test_switch_reader() {
    for (const char* k : {"KBA_STREAM_MIN", "KBA_COOP_MAX_WIN", "KBA_NO_WG_SOLVE", "KBA_NO_COOP_SOLVE", "KBA_COOP_TIMEOUT_MS", "KBA_GROUPS"}) unsetenv(k);
    SolveSwitches s = read_solve_switches();
    CHECK(!s.stream_min_set && s.stream_min == 16 && s.coop_max_win == 64 && !s.no_wg && !s.no_coop && s.coop_timeout_ms == 50.0 && !s.groups_set);
    setenv("KBA_STREAM_MIN", "5", 1);
    setenv("KBA_COOP_MAX_WIN", "1000", 1);
    setenv("KBA_NO_WG_SOLVE", "0", 1);
    setenv("KBA_NO_COOP_SOLVE", "1", 1);
    setenv("KBA_COOP_TIMEOUT_MS", "0", 1);
    setenv("KBA_GROUPS", "9", 1);
    s = read_solve_switches();
    CHECK(s.stream_min_set && s.stream_min == 5 && s.coop_max_win == 256 && !s.no_wg && s.no_coop && s.coop_timeout_ms == 0.0 && s.groups_set && s.groups == 9);
    setenv("KBA_COOP_MAX_WIN", "8", 1);
    setenv("KBA_NO_WG_SOLVE", "1", 1);
    setenv("KBA_COOP_TIMEOUT_MS", "2.5", 1);
    s = read_solve_switches();
    CHECK(s.coop_max_win == 8 && s.no_wg && s.coop_timeout_ms == 2.5);
    for (const char* k : {"KBA_STREAM_MIN", "KBA_COOP_MAX_WIN", "KBA_NO_WG_SOLVE", "KBA_NO_COOP_SOLVE", "KBA_COOP_TIMEOUT_MS", "KBA_GROUPS"}) unsetenv(k);
}

int main() {
    test_plan_table();
    test_worklists();
    test_solve_paths();
    test_stream_geometry();
    test_switch_reader();
    test_lend_guard();
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
