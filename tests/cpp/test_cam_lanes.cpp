// cam_assemble / cam_solve (kba_items.hpp) with 128 lanes that stand in for 256 (nvl = 256: virtual lanes) against 256 lanes: every
// number a window's launch leaves behind must have the same 64-bit pattern - the hand-over region, g_c, the Jacobi scale, the
// regulariser costs, WinRed, the camera step and the candidate poses with their per-view constants.
// The lanes are threads that meet at KBA_SYNC (a pthread barrier), so the host statements run as a workgroup runs them: the
// virtual-lane partial sums, the reduction tree over 256 virtual lanes, the regulariser rows by virtual wave and every index are
// held here under -fsanitize=address,undefined (tests/test_cam_lanes_cpu.py).  The device-only branches (MFMA tiles, readlane
// pivots, one reduction slot per wave) are held on the GPU by tests/test_gpu_cam_lanes.py.
// Stand-alone host program; kba_pack.cpp is part of this translation unit so that one definition of KBA_SYNC holds for all of it.
#include <pthread.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#define KBA_HOST_LANES  // scratch layouts with the host's reduction tree (kba_items.hpp:coop_red_doubles)
static pthread_barrier_t* g_lane_barrier = nullptr;  // the workgroup's barrier while lanes run; null: a single lane
#define KBA_SYNC()                                                 \
    do {                                                           \
        if (g_lane_barrier) pthread_barrier_wait(g_lane_barrier);  \
    } while (0)

#include "../../limo_amd/csrc/kba_pack.cpp"
#include "../../limo_amd/csrc/kba_buffers.hpp"
#include "../../limo_amd/csrc/kba_items.hpp"

using namespace kba;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_failed;                                                    \
            if (g_failed < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

// f(tid) on nt lanes that meet at KBA_SYNC
template <class F>
static void run_lanes(int nt, F f) {
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, (unsigned)nt);
    g_lane_barrier = &bar;
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back([&f, t]() { f(t); });
    for (auto& t : th) t.join();
    g_lane_barrier = nullptr;
    pthread_barrier_destroy(&bar);
}

// ------------------------------------------------------------------------------------------------ windows
struct Win {
    std::vector<double> pose, pdir, pdist, cam, lm, weight;
    std::vector<int32_t> fix, okf, olm, ocam;
    std::vector<uint8_t> ground;
    std::vector<float> u, v, d;
    limo_ba_window w;
};

// n_kf keyframes along the road, n_lm landmarks seen from every keyframe; every third landmark has a depth, every fifth lies on the ground
static void fill(Win& W, int n_kf, int n_lm, unsigned seed) {
    auto rnd = [&seed]() {
        seed = seed * 1664525u + 1013904223u;
        return (double)(seed >> 8) / (double)(1u << 24);
    };
    W.pose.assign((size_t)7 * n_kf, 0.0);
    W.pdir.assign((size_t)3 * n_kf, 0.0);
    W.pdist.assign(n_kf, 0.0);
    W.fix.assign(n_kf, LIMO_FIX_NONE);
    for (int k = 0; k < n_kf; ++k) {
        double q[4] = {1.0, 0.02 * (rnd() - 0.5), 0.05 * (rnd() - 0.5), 0.02 * (rnd() - 0.5)};
        const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int i = 0; i < 4; ++i) W.pose[7 * k + i] = q[i] / qn;
        W.pose[7 * k + 4] = 0.2 * (rnd() - 0.5);
        W.pose[7 * k + 5] = 0.1 * (rnd() - 0.5);
        W.pose[7 * k + 6] = -0.8 * k + 0.1 * rnd();
        double n[3] = {0.03 * (rnd() - 0.5), 1.0, 0.03 * (rnd() - 0.5)};
        const double nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int i = 0; i < 3; ++i) W.pdir[3 * k + i] = n[i] / nn;
        W.pdist[k] = 1.7 + 0.05 * rnd();
    }
    const double cam[10] = {700.0, 600.0, 180.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    W.cam.assign(cam, cam + 10);
    W.lm.resize((size_t)3 * n_lm);
    W.weight.assign(n_lm, 1.0);
    W.ground.assign(n_lm, 0);
    for (int l = 0; l < n_lm; ++l) {
        const bool gr = l % 5 == 2;
        const double x = 8.0 * (rnd() - 0.5), y = gr ? 1.7 : 3.0 * (rnd() - 0.5), z = 6.0 + (gr ? 8.0 : 20.0) * rnd();
        W.lm[3 * l] = x;
        W.lm[3 * l + 1] = y;
        W.lm[3 * l + 2] = z;
        W.ground[l] = gr;
        W.weight[l] = 0.5 + rnd();
        for (int k = 0; k < n_kf; ++k) {
            const double zc = z + W.pose[7 * k + 6];
            W.okf.push_back(k);
            W.olm.push_back(l);
            W.ocam.push_back(0);
            W.u.push_back((float)(700.0 * x / zc + 600.0 + 2.0 * (rnd() - 0.5)));
            W.v.push_back((float)(700.0 * y / zc + 180.0 + 2.0 * (rnd() - 0.5)));
            W.d.push_back(l % 3 == 0 ? (float)(zc + 0.2 * (rnd() - 0.5)) : -1.0f);
        }
    }
    limo_ba_window& w = W.w;
    std::memset(&w, 0, sizeof(w));
    w.n_kf = n_kf;
    w.n_cam = 1;
    w.n_lm = n_lm;
    w.n_obs = (int32_t)W.olm.size();
    w.kf_pose = W.pose.data();
    w.kf_plane_dir = W.pdir.data();
    w.kf_plane_dist = W.pdist.data();
    w.kf_fixation = W.fix.data();
    w.cam = W.cam.data();
    w.lm_pos = W.lm.data();
    w.lm_weight = W.weight.data();
    w.lm_is_ground = W.ground.data();
    w.obs_kf = W.okf.data();
    w.obs_lm = W.olm.data();
    w.obs_cam = W.ocam.data();
    w.obs_u = W.u.data();
    w.obs_v = W.v.data();
    w.obs_d = W.d.data();
}

// ------------------------------------------------------------------------------------------------ linearisation of the batch (one lane)
static void linearize(BatchView& v, const SolveConsts& c) {
    for (int view = 0; view < v.TV; ++view) view_consts_item(v, view);
    for (int w = 0; w < v.n_win; ++w) {
        const WinDesc& wd = v.win[w];
        for (int g = wd.gp0; g < wd.gp0 + wd.n_gp; ++g) gp_lane(v, g, false, v.gp_cost);
    }
    std::vector<LinLane> cam(kMaxViews);
    for (int b = 0; b < v.n_lblk; ++b) {
        const int w = v.lblk_win[b];
        const WinDesc& wd = v.win[w];
        double* out = v.lv_part + wd.lvpart_off + (int64_t)(b - wd.lblk0) * wd.n_view * kLinPartial;
        std::vector<double> slices((size_t)wd.n_view * kLinWaves * kLinPartial, 0.0);
        double gmax = 0.0, xn2 = 0.0;
        int fail = 0;
        for (int t = 0; t < v.lblk_n[b]; ++t) {
            double part[8];
            fail |= lin_lm_lane(v, c, w, v.lblk_lm0[b] + t, v.st[w].first != 0, cam.data(), part);
            gmax = std::fmax(gmax, part[0]);
            xn2 += part[1];
            for (int j = 0; j < wd.n_view; ++j) {
                double* o = slices.data() + ((size_t)j * kLinWaves + t / 64) * kLinPartial;
                for (int i = 0; i < kLinPartial; ++i) o[i] += cam[j].e[i];
            }
        }
        for (int e = 0; e < wd.n_view * kLinPartial; ++e) {
            const double* q = slices.data() + (size_t)(e / kLinPartial) * kLinWaves * kLinPartial + e % kLinPartial;
            out[e] = (q[0] + q[kLinPartial]) + (q[2 * kLinPartial] + q[3 * kLinPartial]);
        }
        v.lblk_part[(int64_t)b * 8 + 0] = gmax;
        v.lblk_part[(int64_t)b * 8 + 1] = xn2;
        v.lblk_linfail[b] = fail;
    }
}

// ------------------------------------------------------------------------------------------------ what a window's two launches leave
struct Left {
    std::vector<double> d;    // every double, in a fixed order
    std::vector<int32_t> i;   // the integers of WinRed
};
static void append(std::vector<double>& v, const double* p, size_t n) { v.insert(v.end(), p, p + n); }

// Scratch of exactly the layout's size (KBA_HOST_LANES: with the reduction tree of the host form, a double per lane and value, where
// the device keeps one slot per wave), so an index that leaves the layout is caught.
static size_t assemble_doubles(const WinDesc& wd, int nvl) { return (size_t)cam_assemble_scratch(wd.nc, nvl, wd.n_view); }
static size_t solve_doubles(const WinDesc& wd, int nvl) { return (size_t)cam_solve_scratch(wd.nc, nvl, wd.nf); }

// cam_assemble + cam_solve of window w with nt lanes (nvl virtual lanes) from the linearisation in bv
static Left run_window(BatchView& bv, const SolveConsts& c, int w, int nt, int nvl, bool compute_scale, double poison) {
    const WinDesc& wd = bv.win[w];
    const int n_need = schur_need_count(wd.nf), n_lanes = nvl > 0 ? nvl : nt;  // (lanes the scratch is laid out for)
    double* Hg = bv.Hcc + wd.hcc_off;
    for (int i = 0; i < wd.nc * wd.nc; ++i) Hg[i] = poison;
    for (int i = 0; i < wd.nc; ++i) bv.gc[wd.cam0 + i] = bv.yc[wd.cam0 + i] = bv.delta_c[wd.cam0 + i] = poison;
    for (int k = wd.kf0; k < wd.kf0 + wd.n_kf; ++k) {
        for (int i = 0; i < 7; ++i) bv.pose_c[7 * k + i] = poison;
        for (int i = 0; i < 3; ++i) bv.pdir_c[3 * k + i] = poison;
        bv.pdist_c[k] = poison;
    }
    for (int j = wd.view0; j < wd.view0 + wd.n_view; ++j)
        for (int i = 0; i < kViewLin; ++i) bv.view_lin_c[(int64_t)kViewLin * j + i] = poison;
    std::memset(&bv.red[w], 0x5a, sizeof(WinRed));
    bv.reg_cost[2 * w] = bv.reg_cost[2 * w + 1] = poison;
    bv.st[w].compute_scale = compute_scale ? 1 : 0;
    bv.st[w].radius = c.initial_radius;
    {
        std::vector<double> scratch(assemble_doubles(wd, n_lanes));
        run_lanes(nt, [&](int tid) { cam_assemble(bv, c, w, tid, nt, scratch.data(), nvl); });
    }
    Left L;
    append(L.d, Hg, (size_t)wd.nc * wd.nc);  // (behind the hand-over: the poison, untouched)
    append(L.d, bv.gc + wd.cam0, wd.nc);
    append(L.d, bv.scale_c + wd.cam0, wd.nc);
    append(L.d, bv.reg_cost + 2 * w, 2);
    CHECK(std::isfinite(bv.red[w].lin_cost) && bv.red[w].lin_cost > 0.0 && !bv.red[w].lin_fail);
    for (int i = n_need; i < wd.nc * wd.nc; ++i) CHECK(std::memcmp(&Hg[i], &poison, 8) == 0);
    {
        std::vector<double> scratch(solve_doubles(wd, n_lanes));
        int flag = 0;
        run_lanes(nt, [&](int tid) { cam_solve(bv, c, w, tid, nt, scratch.data(), &flag, nvl); });
    }
    const WinRed& r = bv.red[w];
    CHECK(r.chol_fail == 0 && std::isfinite(r.mcc) && r.step2 > 0.0);
    const double red[6] = {r.lin_cost, r.gmax, r.xnorm2, r.mcc, r.step2, r.cand2};
    append(L.d, red, 6);
    L.i = {r.lin_fail, r.chol_fail, r.no_variable};
    append(L.d, bv.yc + wd.cam0, wd.nc);
    append(L.d, bv.delta_c + wd.cam0, wd.nc);
    append(L.d, bv.pose_c + 7 * (int64_t)wd.kf0, (size_t)7 * wd.n_kf);
    append(L.d, bv.pdir_c + 3 * (int64_t)wd.kf0, (size_t)3 * wd.n_kf);
    append(L.d, bv.pdist_c + wd.kf0, wd.n_kf);
    append(L.d, bv.view_lin_c + (int64_t)kViewLin * wd.view0, (size_t)kViewLin * wd.n_view);
    return L;
}

int main() {
    limo_ba_options opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.depth_thres = 0.16;
    opts.reprojection_thres = 1.6;
    opts.depth_quantile = 0.95;
    opts.reprojection_quantile = 0.95;
    opts.num_trim_rounds = 1;
    opts.trim_solver_iterations = 2;
    opts.min_landmarks_for_trimming = 100;
    opts.minimum_number_residual_groups = 30;
    opts.max_num_iterations = 100;
    opts.function_tolerance = 1e-6;
    opts.gradient_tolerance = 1e-10;
    opts.parameter_tolerance = 1e-8;
    opts.initial_trust_region_radius = 1e4;
    opts.max_trust_region_radius = 1e16;
    opts.min_trust_region_radius = 1e-32;
    opts.min_lm_diagonal = 1e-6;
    opts.max_lm_diagonal = 1e32;
    opts.min_relative_decrease = 1e-3;
    opts.max_num_consecutive_invalid_steps = 5;
    opts.jacobi_scaling = 1;

    // 2 keyframes: a short system, few entries per lane; 5 keyframes x 700 landmarks: more ground-plane rows (140) and hand-over entries
    // (> 1000) than 128 lanes, so the second virtual lane of a lane has terms of its own in the sums
    const int shape[2][2] = {{2, 60}, {5, 700}};
    std::vector<Win> W(2);
    std::vector<limo_ba_window> wins(2);
    for (int i = 0; i < 2; ++i) {
        fill(W[i], shape[i][0], shape[i][1], 2000u + 31u * i);
        wins[i] = W[i].w;
    }
    PackedBatch P;
    std::string err;
    CHECK(pack_windows(2, wins.data(), opts, PackOptions(), P, err) == LIMO_OK);
    if (g_failed) {
        std::printf("pack failed: %s\n", err.c_str());
        return 1;
    }
    const SolveConsts c = make_consts(opts);
    BatchView bv;
    std::memset(&bv, 0, sizeof(bv));
    std::vector<void*> allocs;
    for_each_buffer(P, bv, [&](void** slot, size_t bytes, const void* init) {
        void* p = std::calloc(1, bytes ? bytes : 1);
        if (init) std::memcpy(p, init, bytes);
        *slot = p;
        allocs.push_back(p);
    });
    for (int w = 0; w < 2; ++w) lm_solve_init(bv.st[w], true, 10, c);
    linearize(bv, c);

    for (int w = 0; w < 2; ++w) {
        const WinDesc& wd = bv.win[w];
        std::printf("window %d: %d keyframes, nc %d, nf %d, %d ground rows, %d regulariser rows, hand-over %d doubles, %d landmark workgroups x %d views\n", w,
                    (int)wd.n_kf, (int)wd.nc, (int)wd.nf, (int)wd.n_gp, reg_row_count(wd), schur_need_count(wd.nf), (int)wd.n_lblk, (int)wd.n_view);
        CHECK(wd.n_kf == shape[w][0] && wd.cam_scr_off < 0 && wd.nc <= kCamLanesHalf);
        if (w == 1) CHECK(wd.n_gp > kCamLanesHalf && schur_need_count(wd.nf) > kBlock);
        for (int pass = 0; pass < 2; ++pass) {  // the linearisation that defines the Jacobi scale, then one that keeps it
            const Left full = run_window(bv, c, w, kBlock, 0, pass == 0, -7.0);
            const Left half = run_window(bv, c, w, kCamLanesHalf, kBlock, pass == 0, -9.0);
            CHECK(full.d.size() == half.d.size() && full.i == half.i);
            const size_t n_hg = (size_t)wd.nc * wd.nc, n_need = (size_t)schur_need_count(wd.nf);
            int n_bad = 0;
            for (size_t i = 0; i < full.d.size() && i < half.d.size(); ++i) {
                if (full.d[i] == -7.0 && half.d[i] == -9.0) {  // the two poisons: a double neither form writes - behind the hand-over, unused view constants
                    CHECK(i >= n_need);
                    continue;
                }
                const bool same = std::memcmp(&full.d[i], &half.d[i], 8) == 0;
                CHECK(same);
                if (!same && ++n_bad < 6) std::printf("  window %d pass %d double %zu: 256 lanes %.17g, 128 lanes %.17g\n", w, pass, i, full.d[i], half.d[i]);
            }
            // (one lane alone - the emulator's form - sums in another order: the comparison above can tell)
            if (w == 1 && pass == 0) {
                const Left one = run_window(bv, c, w, 1, 0, true, -7.0);
                int differ = 0;
                for (size_t i = 0; i < one.d.size(); ++i) differ += i < n_need || i >= n_hg ? std::memcmp(&one.d[i], &full.d[i], 8) != 0 : 0;
                CHECK(differ > 0);
                (void)run_window(bv, c, w, kBlock, 0, true, -7.0);  // (back to the workgroup's scale for the second pass)
            }
        }
    }
    for (void* p : allocs) std::free(p);
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
