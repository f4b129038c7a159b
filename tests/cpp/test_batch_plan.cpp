// Host-only checks of limo_amd/csrc/kba_batch_plan.hpp (the per-batch kernel plan and the Schur worklist builder) and of the pack
// arena's lend guard (kba_pack.hpp:PackArenaLend).  Stand-alone program, built with -fsanitize=address by tests/test_batch_plan_cpu.py
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

int main() {
    test_plan_table();
    test_worklists();
    test_lend_guard();
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
