// Host-only checks of who takes which form of the camera kernels (limo_amd/csrc/kba_batch_plan.hpp: plan_cam_lanes per batch,
// cam_lanes_for_launch per launch, the KBA_CAM_LANES switch of read_solve_switches).  Stand-alone program, built with
// -fsanitize=address,undefined by tests/test_cam_lanes_plan_cpu.py together with kba_pack.cpp.  The expected values are written out
// here, not computed by the code under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static WinDesc window(int n_kf, int64_t cam_scr_off) {
    WinDesc d;
    std::memset(&d, 0, sizeof(d));
    d.n_kf = n_kf;
    d.nc = n_kf * kCamSlots;
    d.nf = d.nc;
    d.cam_scr_off = cam_scr_off;
    return d;
}
static PackedBatch batch_of(const std::vector<WinDesc>& ws) {
    PackedBatch P;
    P.n_win = (int32_t)ws.size();
    P.win = ws;
    return P;
}

int main() {
    CHECK(kBlock == 256 && kCamLanesHalf == 128);
    // ---- per batch.  The device of the model: 256 CUs; assembly 3 / 6 workgroups per CU, solve 4 / 7 (not twice 4: stays at 256 lanes)
    CamOccupancy occ;
    occ.n_cu = 256;
    occ.asm_full = 3;
    occ.asm_half = 6;
    occ.solve_full = 4;
    occ.solve_half = 7;
    {
        const CamLanesPlan p = plan_cam_lanes(batch_of({window(5, -1), window(2, -1)}), occ, true);
        CHECK(p.asm_half_ok && !p.solve_half_ok);
        CHECK(p.asm_resident == 768 && p.solve_resident == 1024);
    }
    occ.solve_half = 8;
    {
        const CamLanesPlan p = plan_cam_lanes(batch_of({window(5, -1), window(2, -1)}), occ, true);
        CHECK(p.asm_half_ok && p.solve_half_ok);
        // a sharded or pose-only batch keeps 256 lanes
        const CamLanesPlan q = plan_cam_lanes(batch_of({window(5, -1)}), occ, false);
        CHECK(!q.asm_half_ok && !q.solve_half_ok && q.asm_resident == 768);
    }
    {   // one window of the global-memory class, or one with more slots than 128 lanes: the whole batch keeps 256 lanes
        const CamLanesPlan p = plan_cam_lanes(batch_of({window(5, -1), window(12, 4096)}), occ, true);
        CHECK(!p.asm_half_ok && !p.solve_half_ok);
        const CamLanesPlan q = plan_cam_lanes(batch_of({window(5, -1), window(13, -1)}), occ, true);  // nc 130
        CHECK(!q.asm_half_ok && !q.solve_half_ok);
        const CamLanesPlan r = plan_cam_lanes(batch_of({window(12, -1)}), occ, true);  // nc 120 in LDS: allowed
        CHECK(r.asm_half_ok && r.solve_half_ok);
        const CamLanesPlan e = plan_cam_lanes(batch_of({}), occ, true);
        CHECK(!e.asm_half_ok && !e.solve_half_ok);
    }
    {   // the runtime reports nothing resident (an LDS size no workgroup fits): never the half form
        CamOccupancy z;
        z.n_cu = 256;
        const CamLanesPlan p = plan_cam_lanes(batch_of({window(5, -1)}), z, true);
        CHECK(!p.asm_half_ok && !p.solve_half_ok && p.asm_resident == 0);
    }
    // ---- the class boundary of the pack stays between 11 and 12 keyframes, although the solve's own scratch at 12 would fit the cap
    CHECK(cam_class_doubles(110, 11) == 18657 && cam_class_doubles(120, 12) == 22152);
    CHECK(cam_class_doubles(110, 11) * 8 <= kCamLdsCapBytes && cam_class_doubles(120, 12) * 8 > kCamLdsCapBytes);
    CHECK(cam_solve_scratch(120, kBlock) == 15012 && cam_solve_scratch(120, kBlock) * 8 < kCamLdsCapBytes);
    CHECK(cam_class_doubles(50, 5) >= cam_assemble_scratch(50, kBlock, 5) && cam_class_doubles(50, 5) >= cam_solve_scratch(50, kBlock));
    // ---- per launch: more windows listed than the 256-lane form holds resident -> 128 lanes
    CHECK(kCamLanesFactor == 1);
    CHECK(cam_lanes_for_launch(true, 768, 4096, 0) == 128);
    CHECK(cam_lanes_for_launch(true, 768, 769, 0) == 128);
    CHECK(cam_lanes_for_launch(true, 768, 768, 0) == 256);
    CHECK(cam_lanes_for_launch(true, 1024, 1024, 0) == 256);
    CHECK(cam_lanes_for_launch(true, 1024, 1, 0) == 256);
    CHECK(cam_lanes_for_launch(false, 768, 4096, 0) == 256);
    // forced: where the batch allows it
    CHECK(cam_lanes_for_launch(true, 768, 16, 128) == 128);
    CHECK(cam_lanes_for_launch(true, 768, 4096, 256) == 256);
    CHECK(cam_lanes_for_launch(false, 768, 16, 128) == 256);
    CHECK(cam_lanes_for_launch(false, 768, 4096, 128) == 256);

    // ---- the switch
    unsetenv("KBA_CAM_LANES");
    CHECK(read_solve_switches().cam_lanes == 0);
    const struct {
        const char* text;
        int want;
    } cases[] = {{"128", 128}, {"256", 256}, {"0", 0}, {"64", 0}, {"", 0}, {"abc", 0}, {"129", 0}, {"-128", 0}};
    for (const auto& cs : cases) {
        setenv("KBA_CAM_LANES", cs.text, 1);
        const SolveSwitches s = read_solve_switches();
        CHECK(s.cam_lanes == cs.want);
        CHECK(!s.gp_wide && !s.groups_set && !s.stream_min_set);  // (nothing else reads it)
    }
    unsetenv("KBA_CAM_LANES");
    setenv("KBA_SCHUR_GP_WIDE", "1", 1);
    CHECK(read_solve_switches().cam_lanes == 0 && read_solve_switches().gp_wide);
    unsetenv("KBA_SCHUR_GP_WIDE");
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
