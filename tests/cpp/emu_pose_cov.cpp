// TEST INFRASTRUCTURE — the emulated pipeline (emu_pipeline.cpp, included as it stands) with an entry that runs the schedule and then
// the covariance pass of limo_hip.h ("Pose covariance") with the kernel's own statement, kba_items.hpp:cam_cov - the pass of
// limo_batch.hpp:PoseCovariance::run in plain loops.  Built by tests/pose_cov_common.py into tests/cpp/_build/libkba_emu_cov.so.
#include "emu_pipeline.cpp"

namespace {

// The Schur slabs of every active window (the first block of EmuBatch::step, which also solves and steps): tile layout, one slab
// per Schur block.
void cov_schur(EmuBatch& B) {
    BatchView& v = B.bv;
    std::vector<double> z;
    for (int sb = 0; sb < v.n_sblk; ++sb) {
        const int w = v.sblk_win[sb];
        if (!v.st[w].active) continue;
        const WinDesc& wd = v.win[w];
        const int nfp = wd.nf_pad, nfq = wd.nfq, slab = nfp * nfp;
        std::vector<int> vkl(wd.n_view);
        for (int j = 0; j < wd.n_view; ++j) vkl[j] = v.view_kf[wd.view0 + j] - wd.kf0;
        double* out = v.S_part + wd.spart_off + (int64_t)(sb - wd.sblk0) * slab;
        for (int i = 0; i < slab; ++i) out[i] = 0.0;
        for (int li = 0; li < v.sblk_n[sb]; ++li) {
            const int gl = v.sblk_lm0[sb] + li;
            if (v.lm_state[gl] != 1) continue;
            double lmk[9], Y[3 * kCamSlots];
            schur_load_lm(v, gl, lmk);
            z.assign((size_t)3 * nfp, 0.0);
            for (int kl = 0; kl < wd.n_kf; ++kl) {
                schur_pair_block(v, wd, gl, kl, lmk, v.scale_c + wd.cam0, vkl.data(), gl >= wd.lm_gp0, Y);
                for (int a = 0; a < kCamSlots; ++a) {
                    const int ci = v.cslot[wd.cam0 + kl * kCamSlots + a];
                    if (ci < 0) continue;
                    for (int cc = 0; cc < 3; ++cc) z[(size_t)cc * nfp + schur_col(ci, nfq)] = Y[a * 3 + cc];
                }
            }
            for (int cc = 0; cc < 3; ++cc) {
                const double* zr = z.data() + (size_t)cc * nfp;
                for (int a = 0; a <= wd.nf; ++a) {
                    if (zr[a] == 0.0) continue;
                    for (int bcol = a; bcol <= wd.nf; ++bcol) out[a * nfp + bcol] += zr[a] * zr[bcol];
                }
            }
        }
    }
}

// The pass: state saved, every window linearised at its final point without damping, Schur slabs, cam_cov, state put back.
void cov_pass(EmuBatch& B, double* cov, int32_t* status) {
    BatchView& bv = B.bv;
    const std::vector<WinState> st_save(bv.st, bv.st + bv.n_win);
    const std::vector<WinRed> red_save(bv.red, bv.red + bv.n_win);
    const SolveConsts keep = B.c;
    B.c.min_lm_diagonal = 0.0;
    B.c.max_lm_diagonal = 0.0;
    B.c.gradient_tolerance = -1.0;
    B.c.min_radius = -1.0;
    for (int w = 0; w < bv.n_win; ++w) {  // k_cov_begin
        WinState& s = bv.st[w];
        s.active = 1;
        s.need_lin = 1;
        s.first = 1;
        s.accept = 0;
        s.compute_scale = 1;
        s.redamp = 0;
        s.radius = 1.0;
        s.iter = 0;
        s.max_iter = 1 << 30;
        s.log = nullptr;
        s.log_cap = 0;
    }
    B.first_lin = true;
    B.linearize();
    cov_schur(B);
    std::vector<double> scratch;
    int64_t off = 0;
    for (int w = 0; w < bv.n_win; ++w) {
        const WinDesc& wd = bv.win[w];
        scratch.assign((size_t)cam_cov_scratch(wd.nf, wd.nfq) + 1, 0.0);
        cam_cov(bv, B.c, w, 0, 1, scratch.data(), cov + off, status + w);
        off += (int64_t)36 * wd.n_kf * wd.n_kf;
    }
    B.c = keep;
    std::memcpy(bv.st, st_save.data(), sizeof(WinState) * st_save.size());
    std::memcpy(bv.red, red_save.data(), sizeof(WinRed) * red_save.size());
}

}  // namespace

extern "C" {

// The windows IN PLACE through the lock-step schedule (n_slots > 0: the streaming schedule), then the pass.  lm_fixed: NULL, or n
// entries, each NULL or that window's n_lm flags.  cov: sum (6 n_kf)^2 doubles, the windows' matrices back to back; status: n.
int emu_ba_solve_batch_cov(int32_t n, limo_ba_window* windows, const uint8_t* const* lm_fixed, const limo_ba_options* o, limo_ba_report* reports,
                           int pose_only, const limo_speed_prior* prior, int n_slots, double* cov, int32_t* status) {
    EmuBatch B;
    std::string err;
    PackOptions po;
    po.pose_only = pose_only != 0;
    po.prior = prior;
    po.lm_fixed = lm_fixed;
    int rc = pack_windows(n, windows, *o, po, B.P, err);
    if (rc != LIMO_OK) return rc;
    B.c = make_consts(*o);
    B.alloc();
    if (n_slots > 0)
        B.run_streaming(n_slots);
    else
        run_schedule(B, *o);
    write_back(B, windows);
    record_trimmed(B);
    if (reports)
        for (int w = 0; w < n; ++w) fill_report(B, w, reports + w);
    cov_pass(B, cov, status);
    // the pass is invisible: the report after it is the report before it
    if (reports)
        for (int w = 0; w < n; ++w) {
            limo_ba_report again;
            fill_report(B, w, &again);
            if (std::memcmp(&again, reports + w, sizeof(again)) != 0) return LIMO_ERR_RUNTIME;
        }
    return LIMO_OK;
}

}  // extern "C"
