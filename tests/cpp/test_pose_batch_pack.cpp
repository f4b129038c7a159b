// Host-only checks of the per-window speed prior of a pose-only batch (kba_pack.hpp:PackOptions::per_window_prior / window_priors,
// what limo_ba_batch_create_pose_only packs with).  Stand-alone program, built with -fsanitize=address by
// tests/test_pose_batch_pack_cpu.py together with kba_pack.cpp.  Every window of a batch must be described exactly as the same
// window packed alone through the single-window interface (PackOptions::prior), apart from its place in the batch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../limo_amd/csrc/kba_pack.hpp"

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

// One frame against fixed landmarks: n_lm landmarks in front of one camera, every landmark observed once except every
// `skip`-th one (those stay out of the problem: lm_state 0).
struct Win {
    std::vector<double> pose, pdir, pdist, cam, lm, weight;
    std::vector<int32_t> fix, okf, olm, ocam;
    std::vector<uint8_t> ground;
    std::vector<float> u, v, d;
    std::vector<uint8_t> observed;
    limo_ba_window w;
};

static void fill(Win& W, int n_kf, int n_lm, int skip, unsigned seed) {
    auto rnd = [&seed]() {
        seed = seed * 1664525u + 1013904223u;
        return (double)(seed >> 8) / (double)(1u << 24);
    };
    W.pose.assign((size_t)7 * n_kf, 0.0);
    for (int k = 0; k < n_kf; ++k) {
        W.pose[7 * k] = 1.0;
        W.pose[7 * k + 4] = 0.1 * rnd();
        W.pose[7 * k + 6] = 0.2 * rnd();
    }
    W.pdir.assign((size_t)3 * n_kf, 0.0);
    for (int k = 0; k < n_kf; ++k) W.pdir[3 * k + 1] = 1.0;
    W.pdist.assign(n_kf, 1.7);
    W.fix.assign(n_kf, LIMO_FIX_NONE);
    W.cam = {700.0, 600.0, 180.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    W.lm.resize((size_t)3 * n_lm);
    W.weight.assign(n_lm, 1.0);
    W.ground.assign(n_lm, 0);
    W.observed.assign(n_lm, 0);
    W.okf.clear();
    W.olm.clear();
    W.ocam.clear();
    W.u.clear();
    W.v.clear();
    W.d.clear();
    for (int l = 0; l < n_lm; ++l) {
        const double x = 8.0 * (rnd() - 0.5), y = 3.0 * (rnd() - 0.5), z = 5.0 + 20.0 * rnd();
        W.lm[3 * l] = x;
        W.lm[3 * l + 1] = y;
        W.lm[3 * l + 2] = z;
        if (l % 7 == 3) W.ground[l] = 1;  // (ground flags are ignored by a pose-only problem)
        if (skip > 0 && l % skip == skip - 1) continue;
        W.observed[l] = 1;
        W.okf.push_back(0);
        W.olm.push_back(l);
        W.ocam.push_back(0);
        W.u.push_back((float)(700.0 * x / z + 600.0 + rnd()));
        W.v.push_back((float)(700.0 * y / z + 180.0 + rnd()));
        W.d.push_back(l % 3 == 0 ? (float)z : -1.0f);
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

static limo_speed_prior prior_of(int i, double weight) {
    limo_speed_prior p;
    std::memset(&p, 0, sizeof(p));
    p.speed_weight = weight;
    p.dt_cur = 0.1 + 0.05 * i;
    for (int q = 0; q < 3; ++q) p.vel_prev[q] = 1.0 + i + 0.25 * q;
    // a rotation about y by 0.1 (i + 1) rad; window 0: the identity
    const double a = i == 0 ? 0.0 : 0.1 * (i + 1);
    p.pose_before[0] = std::cos(a / 2);
    p.pose_before[2] = std::sin(a / 2);
    for (int q = 0; q < 3; ++q) p.pose_before[4 + q] = 0.5 * i - q;
    return p;
}

// The descriptor of window w of a batch with its place in the batch taken out: what packing the window alone must give.
static WinDesc without_offsets(const WinDesc& in, const std::vector<WinDesc>& alone, int w) {
    WinDesc d;
    std::memcpy(&d, &in, sizeof(d));
    int64_t K = 0, L = 0, V = 0, O = 0, B = 0, LB = 0, H = 0, X = 0, LV = 0;
    for (int i = 0; i < w; ++i) {
        const WinDesc& a = alone[i];
        K += a.n_kf;
        L += a.n_lm;
        V += a.n_view;
        O += a.n_obs;
        B += a.n_blk;
        LB += a.n_lblk;
        H += (int64_t)a.nc * a.nc;
        X += (int64_t)a.n_view * kLinPartial;
        LV += (int64_t)a.n_lblk * a.n_view * kLinPartial;
    }
    d.kf0 -= (int32_t)K;
    d.cam0 -= (int32_t)K * kCamSlots;
    d.lm0 -= (int32_t)L;
    d.lm_gp0 -= (int32_t)L;
    d.view0 -= (int32_t)V;
    for (int q = 0; q < 4; ++q)
        if (d.fk_view[q] >= 0) d.fk_view[q] -= (int32_t)V;
    d.obs0 -= (int32_t)O;
    d.blk0 -= (int32_t)B;
    d.lblk0 -= (int32_t)LB;
    d.hcc_off -= H;
    d.xlv_off -= X;
    d.lvpart_off -= LV;
    return d;
}

int main() {
    limo_ba_options opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.min_landmarks_for_trimming = 30;  // (what adjustPoseOnly uses; nothing else of the options is read by the packer)
    const int n = 5;
    // 300 landmarks: two landmark workgroups; 12 and 30: no trimming (n_lm > 30 trims); 31: the first size that trims
    const int n_lm[n] = {40, 300, 12, 31, 30}, skip[n] = {0, 9, 4, 0, 5};
    std::vector<Win> W(n);
    for (int i = 0; i < n; ++i) fill(W[i], 1, n_lm[i], skip[i], 100u + i);
    std::vector<limo_ba_window> wins(n);
    for (int i = 0; i < n; ++i) wins[i] = W[i].w;
    // priors on windows 0, 2 and 4; speed_weight = 0 on window 1 and a negative one on window 3: no prior there
    const double weight[n] = {0.7, 0.0, 0.4, -1.0, 0.9};
    std::vector<limo_speed_prior> priors(n);
    for (int i = 0; i < n; ++i) priors[i] = prior_of(i, weight[i]);

    std::string err;
    std::vector<WinDesc> alone(n);
    std::vector<PackedBatch> Pa(n);
    for (int i = 0; i < n; ++i) {  // the single call's way: PackOptions::prior
        PackOptions po;
        po.pose_only = true;
        po.prior = &priors[i];
        CHECK(pack_windows(1, &wins[i], opts, po, Pa[i], err) == LIMO_OK);
        alone[i] = Pa[i].win[0];
    }
    PackedBatch P;
    {
        PackOptions po;
        po.pose_only = true;
        po.per_window_prior = true;
        po.window_priors = priors.data();
        po.prior = &priors[4];  // (must be ignored by a per-window batch)
        CHECK(pack_windows(n, wins.data(), opts, po, P, err) == LIMO_OK);
    }
    CHECK(P.n_win == n && (int)P.win.size() == n);
    int32_t kf0 = 0, lm0 = 0, view0 = 0, obs0 = 0, blk0 = 0, lblk0 = 0;
    for (int i = 0; i < n && (int)P.win.size() == n; ++i) {
        const WinDesc& d = P.win[i];
        const WinDesc& a = alone[i];
        // consistent prefix sums
        CHECK(d.kf0 == kf0 && d.lm0 == lm0 && d.view0 == view0 && d.obs0 == obs0 && d.blk0 == blk0 && d.lblk0 == lblk0);
        CHECK(d.cam0 == kf0 * kCamSlots && d.sblk0 == 0 && d.n_sblk == 0 && d.gp0 == 0 && d.n_gp == 0);
        kf0 += d.n_kf;
        lm0 += d.n_lm;
        view0 += d.n_view;
        obs0 += d.n_obs;
        blk0 += d.n_blk;
        lblk0 += d.n_lblk;
        // the fields the solve reads, one by one ...
        CHECK(d.pose_only == 1 && a.pose_only == 1);
        CHECK(d.do_trim == a.do_trim && d.do_trim == (n_lm[i] > 30 ? 1 : 0));
        CHECK(d.n_lblk == a.n_lblk && d.n_lblk == (n_lm[i] + kBlock - 1) / kBlock);
        CHECK(d.n_kf == 1 && d.n_lm == n_lm[i] && d.n_view == 1 && d.n_obs == W[i].w.n_obs && d.nf == 6 && d.nfq == 6);
        CHECK(d.speed_w == a.speed_w && d.speed_dt == a.speed_dt);
        CHECK(std::memcmp(d.speed_vel, a.speed_vel, sizeof(d.speed_vel)) == 0);
        CHECK(std::memcmp(d.speed_Rb, a.speed_Rb, sizeof(d.speed_Rb)) == 0);
        CHECK(std::memcmp(d.speed_tb, a.speed_tb, sizeof(d.speed_tb)) == 0);
        // ... against the caller's prior itself ...
        if (weight[i] > 0.0) {
            CHECK(d.speed_w == weight[i] && d.speed_dt == priors[i].dt_cur);
            for (int q = 0; q < 3; ++q) CHECK(d.speed_vel[q] == priors[i].vel_prev[q] && d.speed_tb[q] == priors[i].pose_before[4 + q]);
        } else {
            CHECK(d.speed_w == 0.0 && d.speed_dt == 0.0);
            for (int q = 0; q < 9; ++q) CHECK(d.speed_Rb[q] == 0.0);
        }
        // ... and the whole descriptor
        const WinDesc r = without_offsets(d, alone, i);
        CHECK(std::memcmp(&r, &a, sizeof(WinDesc)) == 0);
        // landmark states: 2 (constant, in the problem) for every observed landmark, 0 for the others; same parameters as alone
        for (int l = 0; l < d.n_lm; ++l) {
            const int id = P.lm_id[d.lm0 + l];
            CHECK(id == Pa[i].lm_id[l]);
            CHECK(P.lm_state[d.lm0 + l] == (W[i].observed[id] ? 2 : 0));
            CHECK(P.lm_state[d.lm0 + l] == Pa[i].lm_state[l]);
        }
        CHECK(std::memcmp(P.pose.data() + 7 * (size_t)d.kf0, Pa[i].pose.data(), sizeof(double) * 7) == 0);
        CHECK(std::memcmp(P.lm.data() + 3 * (size_t)d.lm0, Pa[i].lm.data(), sizeof(double) * 3 * d.n_lm) == 0);
        CHECK(std::memcmp(P.obs_u.data() + d.obs0, Pa[i].obs_u.data(), sizeof(float) * d.n_obs) == 0);
        for (int o = 0; o < d.n_obs; ++o) CHECK(P.obs_lm[d.obs0 + o] - d.lm0 == Pa[i].obs_lm[o] && P.obs_src[d.obs0 + o] == Pa[i].obs_src[o]);
    }
    if ((int)P.win.size() == n) {  // window 0's prior has the identity rotation, window 2's is written out: R_y(0.3)
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int q = 0; q < 9; ++q) CHECK(std::fabs(P.win[0].speed_Rb[q] - I[q]) < 1e-15);
        const double c = std::cos(0.3), s = std::sin(0.3);
        const double Ry[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
        for (int q = 0; q < 9; ++q) CHECK(std::fabs(P.win[2].speed_Rb[q] - Ry[q]) < 1e-15);
    }
    CHECK(P.TK == n && P.TL == lm0 && P.TO == obs0 && P.n_lblk == lblk0 && P.n_blk == blk0 && P.n_sblk == 0 && P.TG == 0);

    {   // a NULL priors array = every prior disabled
        PackedBatch Pn, Pz;
        PackOptions po;
        po.pose_only = true;
        po.per_window_prior = true;
        po.prior = &priors[0];  // (ignored)
        CHECK(pack_windows(n, wins.data(), opts, po, Pn, err) == LIMO_OK);
        std::vector<limo_speed_prior> off(priors);
        for (auto& p : off) p.speed_weight = 0.0;
        po.window_priors = off.data();
        CHECK(pack_windows(n, wins.data(), opts, po, Pz, err) == LIMO_OK);
        CHECK(Pn.win.size() == Pz.win.size() && (int)Pn.win.size() == n);
        for (size_t i = 0; i < Pn.win.size() && i < Pz.win.size(); ++i) {
            CHECK(std::memcmp(&Pn.win[i], &Pz.win[i], sizeof(WinDesc)) == 0);
            CHECK(Pn.win[i].speed_w == 0.0);
        }
        CHECK(Pn.lm_state.size() == Pz.lm_state.size() && std::memcmp(Pn.lm_state.data(), Pz.lm_state.data(), Pn.lm_state.size()) == 0);
    }
    {   // an invalid window fails the whole batch, and the error names it
        Win bad;
        fill(bad, 2, 20, 0, 7u);
        std::vector<limo_ba_window> ws(wins);
        ws[3] = bad.w;
        PackedBatch Pb;
        PackOptions po;
        po.pose_only = true;
        po.per_window_prior = true;
        po.window_priors = priors.data();
        std::string e;
        CHECK(pack_windows(n, ws.data(), opts, po, Pb, e) == LIMO_ERR_INVALID);
        CHECK(e.find("window 3") != std::string::npos);
        CHECK(e.find("exactly one keyframe") != std::string::npos);
        // an observation index out of range in window 1
        ws = wins;
        std::vector<int32_t> olm(W[1].olm);
        olm[5] = n_lm[1];
        ws[1].obs_lm = olm.data();
        e.clear();
        CHECK(pack_windows(n, ws.data(), opts, po, Pb, e) == LIMO_ERR_INVALID);
        CHECK(e.find("window 1") != std::string::npos);
        // the single-window interface keeps its messages
        PackOptions p1;
        p1.pose_only = true;
        e.clear();
        CHECK(pack_windows(1, &bad.w, opts, p1, Pb, e) == LIMO_ERR_INVALID);
        CHECK(e == "pose-only window must hold exactly one keyframe");
        e.clear();
        CHECK(pack_windows(0, wins.data(), opts, po, Pb, e) == LIMO_ERR_INVALID);
        CHECK(pack_windows(n, nullptr, opts, po, Pb, e) == LIMO_ERR_INVALID);
    }
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
