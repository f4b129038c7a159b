// What cam_assemble hands to cam_solve (kba_items.hpp): the entries S_c H S_c | S_c g_c of the free slots, in the solve's
// enumeration, at the head of the window's Hcc region.  cam_assemble keeps H as the block tridiagonal band it is by construction
// (cam_bt_index); this program holds its own restatement of the DENSE assembly - zero an nc x nc matrix, add the observation sums,
// the ground-plane rows and the regulariser rows (with their mirror images), mask the constant slots, then enumerate
// sc[a] * sc[b] * H[a][b] - and compares every entry of the hand-over with it as a 64-bit pattern.
// Stand-alone host program (tests/test_cam_handover_cpu.py builds it with -fsanitize=address,undefined together with kba_pack.cpp):
// the scratch vectors have exactly cam_assemble_scratch / cam_solve_scratch doubles, so an index that leaves the layout is caught.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// ------------------------------------------------------------------------------------------------ windows
struct Win {
    std::vector<double> pose, pdir, pdist, cam, lm, weight;
    std::vector<int32_t> fix, okf, olm, ocam;
    std::vector<uint8_t> ground;
    std::vector<float> u, v, d;
    limo_ba_window w;
};

// n_kf keyframes along the road, n_lm landmarks seen from every keyframe (camera (l + k) mod n_cam); every third landmark has a
// depth, every fifth lies on the ground (none when `ground` is off).
static void fill(Win& W, int n_kf, int n_lm, int n_cam, bool ground, const int* fixation, unsigned seed) {
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
        if (fixation) W.fix[k] = fixation[k];
    }
    W.cam.clear();
    for (int c = 0; c < n_cam; ++c) {
        const double a = 0.1 * c;  // camera c looks a little to the side
        const double cam[10] = {700.0 + 10.0 * c, 600.0, 180.0, std::cos(a / 2), 0.0, std::sin(a / 2), 0.0, 0.3 * c, 0.0, 0.0};
        W.cam.insert(W.cam.end(), cam, cam + 10);
    }
    W.lm.resize((size_t)3 * n_lm);
    W.weight.assign(n_lm, 1.0);
    W.ground.assign(n_lm, 0);
    for (int l = 0; l < n_lm; ++l) {
        const bool gr = ground && l % 5 == 2;
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
            W.ocam.push_back((l + k) % n_cam);
            W.u.push_back((float)(700.0 * x / zc + 600.0 + 2.0 * (rnd() - 0.5)));
            W.v.push_back((float)(700.0 * y / zc + 180.0 + 2.0 * (rnd() - 0.5)));
            W.d.push_back(l % 3 == 0 ? (float)(zc + 0.2 * (rnd() - 0.5)) : -1.0f);
        }
    }
    limo_ba_window& w = W.w;
    std::memset(&w, 0, sizeof(w));
    w.n_kf = n_kf;
    w.n_cam = n_cam;
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

// ------------------------------------------------------------------------------------------------ the dense assembly, restated
// H (nc x nc, dense) and g_c of window w from the linearisation in bv, then the enumeration the solve reads: out[i], i in
// [0, schur_need_count(nf)).  sc: the Jacobi scale to use when compute_scale is off; receives the scale computed otherwise.
static void dense_handover(const BatchView& bv, const SolveConsts& c, int w, bool compute_scale, std::vector<double>& sc, std::vector<double>& out) {
    const WinDesc& wd = bv.win[w];
    const int nc = wd.nc;
    std::vector<double> H((size_t)nc * nc, 0.0), gc(nc, 0.0);
    // (1) observations
    std::vector<double> raw((size_t)wd.n_view * kLinPartial);
    for (int e = 0; e < wd.n_view * kLinPartial; ++e) {
        const double* lp = bv.lv_part + wd.lvpart_off + e;
        const int64_t stride = (int64_t)wd.n_view * kLinPartial;
        double acc = 0.0;
        for (int b = 0; b < wd.n_lblk; ++b) acc += lp[b * stride];
        raw[e] = acc;
    }
    for (int kl = 0; kl < wd.n_kf; ++kl)
        for (int q = 0; q < 27; ++q) {
            double acc = 0.0;
            for (int j = 0; j < wd.n_view; ++j) {
                if (bv.view_kf[wd.view0 + j] - wd.kf0 != kl) continue;
                acc += cam_raw_entry(q, raw.data() + j * kLinPartial, bv.view_cam + 16 * (int64_t)(wd.view0 + j) + 4);
            }
            if (q < 21) {
                int a = 0, rem = q;
                while (rem >= 6 - a) {
                    rem -= 6 - a;
                    ++a;
                }
                const int bb = a + rem;
                H[(size_t)(kl * kCamSlots + a) * nc + kl * kCamSlots + bb] += acc;
                if (bb != a) H[(size_t)(kl * kCamSlots + bb) * nc + kl * kCamSlots + a] += acc;
            } else {
                gc[kl * kCamSlots + (q - 21)] += acc;
            }
        }
    // (2) ground-plane rows, in chunks of kGpChunk rows
    for (int g0 = wd.gp0; g0 < wd.gp0 + wd.n_gp; g0 += kGpChunk) {
        const int ng = std::min(kGpChunk, wd.gp0 + wd.n_gp - g0);
        for (int kl = 0; kl < wd.n_kf; ++kl)
            for (int q = 0; q < 110; ++q) {
                const int a = q < 100 ? q / 10 : q - 100, bb = q < 100 ? q % 10 : 10;
                int lo = bv.kf_gp0[wd.kf0 + kl] - g0, hi = lo + bv.kf_ngp[wd.kf0 + kl];
                lo = lo < 0 ? 0 : lo;
                hi = hi > ng ? ng : hi;
                double acc = 0.0;
                for (int g = lo; g < hi; ++g) {
                    const double va = bv.gp_F[(int64_t)a * bv.SG + g0 + g];
                    const double vb = bb < 10 ? bv.gp_F[(int64_t)bb * bv.SG + g0 + g] : bv.gp_r[g0 + g];
                    acc += va * vb;
                }
                if (bb < 10)
                    H[(size_t)(kl * kCamSlots + a) * nc + kl * kCamSlots + bb] += acc;
                else
                    gc[kl * kCamSlots + a] += acc;
            }
    }
    // (3) regulariser rows
    const int nrows = reg_row_count(wd);
    std::vector<double> dense((size_t)std::max(1, nrows) * kRegDense, 0.0);
    for (int i = 0; i < nrows; ++i) {
        RegRow row;
        int all_const;
        reg_row_eval(wd, bv.cmask, bv.pose, bv.pdir, bv.pdist, i, true, row, all_const);
        if (all_const) row.n = -1;
        double* dd = dense.data() + (size_t)i * kRegDense;
        int klo = 1 << 20;
        for (int p = 0; p < row.n; ++p) klo = std::min(klo, row.col[p] / kCamSlots);
        if (row.n <= 0) klo = -(1 << 20);
        for (int p = 0; p < row.n; ++p) dd[2 + row.col[p] - klo * kCamSlots] = row.val[p];
        dd[0] = row.r;
        dd[1] = (double)klo;
    }
    for (int blk = 0; blk < 2 * wd.n_kf - 1; ++blk)
        for (int q = 0; q < kCamSlots * kCamSlots; ++q) {
            const int ka = blk < wd.n_kf ? blk : blk - wd.n_kf, kb = blk < wd.n_kf ? blk : ka + 1;
            const int a = ka * kCamSlots + q / kCamSlots, b = kb * kCamSlots + q % kCamSlots;
            double acc = H[(size_t)a * nc + b];
            reg_rows_of_block(wd, ka, kb, [&](int lo, int cnt, int base) {
                const double* da = dense.data() + (size_t)lo * kRegDense + 2 + a - base * kCamSlots;
                const double* db = dense.data() + (size_t)lo * kRegDense + 2 + b - base * kCamSlots;
                for (int i = 0; i < cnt; ++i) acc += da[i * kRegDense] * db[i * kRegDense];
            });
            H[(size_t)a * nc + b] = acc;
            if (ka != kb) H[(size_t)b * nc + a] = acc;
        }
    for (int a = 0; a < nc; ++a) {
        double acc = gc[a];
        reg_rows_of_block(wd, a / kCamSlots, a / kCamSlots, [&](int lo, int cnt, int base) {
            const double* da = dense.data() + (size_t)lo * kRegDense + 2 + a - base * kCamSlots;
            const double* dr = dense.data() + (size_t)lo * kRegDense;
            for (int i = 0; i < cnt; ++i) acc += da[i * kRegDense] * dr[i * kRegDense];
        });
        gc[a] = acc;
    }
    // (4) mask, scale
    const uint8_t* cm = bv.cmask + (int64_t)wd.cam0;
    for (int i = 0; i < nc * nc; ++i)
        if (!cm[i / nc] || !cm[i % nc]) H[i] = 0.0;
    for (int i = 0; i < nc; ++i)
        if (!cm[i]) gc[i] = 0.0;
    if (compute_scale) {
        sc.assign(nc, 1.0);
        for (int i = 0; i < nc; ++i) sc[i] = (cm[i] && c.jacobi_scaling) ? 1.0 / (1.0 + std::sqrt(H[(size_t)i * nc + i])) : 1.0;
    }
    // what the solve read: free slot ca -> slot fl[ca]; upper triangle + rhs, row by row
    std::vector<int> fl(wd.nf, -1);
    for (int a = 0; a < nc; ++a)
        if (bv.cslot[wd.cam0 + a] >= 0) fl[bv.cslot[wd.cam0 + a]] = a;
    out.clear();
    for (int ca = 0; ca < wd.nf; ++ca)
        for (int cb = ca; cb <= wd.nf; ++cb) {
            const int a = fl[ca];
            if (cb < wd.nf) {
                const int b = fl[cb];
                out.push_back(sc[a] * sc[b] * H[(size_t)a * nc + b]);
            } else {
                out.push_back(sc[a] * gc[a]);
            }
        }
}

// ------------------------------------------------------------------------------------------------ linearisation of the batch
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

int main() {
    // ---- cam_bt_index: a bijection of the band onto [0, 55 n_kf + 100 (n_kf - 1)), the same place for an entry and its mirror image, -1 outside
    for (int nkf = 1; nkf <= 20; ++nkf) {
        const int nc = nkf * kCamSlots, n = 55 * nkf + 100 * (nkf - 1);
        CHECK(cam_bt_count(nc) == n);
        std::vector<int> hit(n, 0);
        bool ok = true, sym = true, outside = true;
        for (int a = 0; a < nc; ++a)
            for (int b = 0; b < nc; ++b) {
                const int e = cam_bt_index(nc, a, b), ka = a / kCamSlots, kb = b / kCamSlots;
                if (std::abs(ka - kb) > 1) {
                    outside = outside && e == -1;
                    continue;
                }
                if (e < 0 || e >= n) {
                    ok = false;
                    continue;
                }
                sym = sym && e == cam_bt_index(nc, b, a);
                if (a <= b) ++hit[e];
            }
        for (int e = 0; e < n; ++e) ok = ok && hit[e] == 1;
        CHECK(ok);
        CHECK(sym);
        CHECK(outside);
    }

    // ---- the hand-over of seven windows against the dense restatement
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

    const int fix4[4] = {LIMO_FIX_POSE, LIMO_FIX_NONE, LIMO_FIX_POSE, LIMO_FIX_NONE};
    struct Shape {
        const char* name;
        int n_kf, n_lm, n_cam;
        bool ground;
        const int* fixation;
    };
    const Shape shapes[] = {
        {"one keyframe", 1, 40, 1, true, nullptr},
        {"two keyframes", 2, 45, 1, true, nullptr},
        {"five keyframes (C2 kind)", 5, 60, 1, true, nullptr},
        {"fixation POSE NONE POSE NONE", 4, 50, 1, true, fix4},
        {"no ground plane", 3, 48, 1, false, nullptr},
        {"two cameras per keyframe", 3, 52, 2, true, nullptr},
        {"13 keyframes", 13, 56, 1, true, nullptr},
    };
    const int n = (int)(sizeof(shapes) / sizeof(shapes[0]));
    std::vector<Win> W(n);
    std::vector<limo_ba_window> wins(n);
    for (int i = 0; i < n; ++i) {
        fill(W[i], shapes[i].n_kf, shapes[i].n_lm, shapes[i].n_cam, shapes[i].ground, shapes[i].fixation, 1000u + 17u * i);
        wins[i] = W[i].w;
    }
    PackedBatch P;
    std::string err;
    CHECK(pack_windows(n, wins.data(), opts, PackOptions(), P, err) == LIMO_OK);
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
    for (int w = 0; w < n; ++w) lm_solve_init(bv.st[w], true, 10, c);
    linearize(bv, c);

    for (int w = 0; w < n; ++w) {
        const WinDesc& wd = bv.win[w];
        const int n_need = schur_need_count(wd.nf);
        std::printf("window %d (%s): nc %d, nf %d (pose slots %d), %d ground rows, %d regulariser rows, hand-over %d doubles, band %d of %d\n", w,
                    shapes[w].name, (int)wd.nc, (int)wd.nf, (int)wd.nfq, (int)wd.n_gp, reg_row_count(wd), n_need, cam_bt_count(wd.nc), wd.nc * wd.nc);
        CHECK(wd.n_kf == shapes[w].n_kf && wd.nc == wd.n_kf * kCamSlots);
        CHECK((wd.n_gp > 0) == shapes[w].ground);
        CHECK(n_need <= wd.nc * wd.nc);
        CHECK(wd.nf > 0);
        if (shapes[w].fixation) CHECK(wd.nf < wd.nc && bv.cslot[wd.cam0] < 0 && bv.cslot[wd.cam0 + kCamSlots] >= 0);
        double* Hg = bv.Hcc + wd.hcc_off;
        for (int pass = 0; pass < 2; ++pass) {
            // pass 0: the linearisation that defines the Jacobi scale; pass 1: a later one, the scale comes from bv.scale_c
            const bool compute_scale = pass == 0;
            bv.st[w].compute_scale = compute_scale ? 1 : 0;
            if (pass == 1)  // (another scale than the one H gives, so that a hand-over that recomputed it would differ)
                for (int i = 0; i < wd.nc; ++i)
                    if (bv.cmask[wd.cam0 + i]) bv.scale_c[wd.cam0 + i] *= 1.0 + 0.01 * (i % 7);
            std::vector<double> sc(bv.scale_c + wd.cam0, bv.scale_c + wd.cam0 + wd.nc), ref;
            dense_handover(bv, c, w, compute_scale, sc, ref);
            CHECK((int)ref.size() == n_need);
            for (int i = 0; i < wd.nc * wd.nc; ++i) Hg[i] = -7.0;  // (whatever an earlier linearisation left)
            {
                std::vector<double> scratch((size_t)cam_assemble_scratch(wd.nc, 1, wd.n_view));  // exactly what the layout asks for
                cam_assemble(bv, c, w, 0, 1, scratch.data());
            }
            int n_zero = 0, n_bad = 0;
            for (int i = 0; i < n_need; ++i) {
                if (!same_bits(Hg[i], ref[i])) {
                    if (++n_bad < 5) std::printf("  entry %d: %.17g, dense assembly %.17g\n", i, Hg[i], ref[i]);
                }
                n_zero += same_bits(Hg[i], 0.0);
            }
            CHECK(n_bad == 0);
            for (int i = n_need; i < wd.nc * wd.nc; ++i) CHECK(same_bits(Hg[i], -7.0));  // nothing behind the hand-over is written
            if (wd.n_kf >= 3) CHECK(n_zero > 0);  // (entries outside the band exist and are +0.0)
            if (compute_scale)
                for (int i = 0; i < wd.nc; ++i) CHECK(same_bits(bv.scale_c[wd.cam0 + i], sc[i]));
            CHECK(std::isfinite(bv.red[w].lin_cost) && bv.red[w].lin_cost > 0.0 && !bv.red[w].lin_fail);
            // ... and the solve takes it from there: scratch of exactly cam_solve_scratch doubles, no slab yet (S_part is zero), so the
            // system is S_c H S_c + D and must factorise
            bv.st[w].radius = c.initial_radius;
            {
                std::vector<double> scratch((size_t)cam_solve_scratch(wd.nc, 1, wd.nf));
                int flag = 0;
                cam_solve(bv, c, w, 0, 1, scratch.data(), &flag);
            }
            CHECK(bv.red[w].chol_fail == 0);
            CHECK(std::isfinite(bv.red[w].mcc) && bv.red[w].step2 > 0.0);
            for (int i = 0; i < n_need; ++i) CHECK(same_bits(Hg[i], ref[i]));  // the solve leaves the hand-over as it is (a rejected step reads it again)
        }
    }
    for (void* p : allocs) std::free(p);
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
