// TEST INFRASTRUCTURE — the emulated pipeline (emu_pipeline.cpp, included as it stands) with an entry that takes per-landmark
// constness flags: what limo_ba_solve_fixed_landmarks / limo_ba_batch_create_fixed_landmarks hand to the packer
// (PackOptions::lm_fixed).  Built by tests/fixed_lm_common.py into tests/cpp/_build/libkba_emu_fixed.so.
#include "emu_pipeline.cpp"

extern "C" {

// lm_fixed: NULL, or n entries, each NULL or that window's n_lm flags.  n_slots > 0: the streaming schedule with that many windows in
// flight, else the lock-step schedule.  The trimmed landmarks of the windows: emu_last_trimmed.
int emu_ba_solve_batch_fixed(int32_t n, limo_ba_window* windows, const uint8_t* const* lm_fixed, const limo_ba_options* o, limo_ba_report* reports,
                             int n_slots) {
    EmuBatch B;
    std::string err;
    PackOptions po;
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
    return LIMO_OK;
}

// The packed layout of ONE window (flags: NULL or n_lm entries), for the pack tests.  Outputs (any may be NULL):
//   counts[8]  n_lm_const, n_lblk, n_sblk, n_sblk_plain, lm_gp0 - lm0, n_gp, n_view_fixed0, nf
//   lm_id / lm_state / lm_gp [n_lm]   packed order
//   lblk / sblk [2 * cap]             (first packed landmark, count) per block, at most cap of them
int emu_pack_layout(const limo_ba_window* window, const uint8_t* flags, const limo_ba_options* o, int32_t* counts, int32_t* lm_id,
                    uint8_t* lm_state, int32_t* lm_gp, int32_t cap, int32_t* lblk, int32_t* sblk) {
    PackedBatch P;
    std::string err;
    PackOptions po;
    const uint8_t* one[1] = {flags};
    po.lm_fixed = flags ? one : nullptr;
    int rc = pack_windows(1, window, *o, po, P, err);
    if (rc != LIMO_OK) return rc;
    const WinDesc& d = P.win[0];
    if (counts) {
        const int32_t c[8] = {d.n_lm_const, d.n_lblk, d.n_sblk, d.n_sblk_plain, d.lm_gp0 - d.lm0, d.n_gp, d.n_view_fixed0, d.nf};
        std::memcpy(counts, c, sizeof(c));
    }
    for (int l = 0; l < d.n_lm; ++l) {
        if (lm_id) lm_id[l] = P.lm_id[l];
        if (lm_state) lm_state[l] = P.lm_state[l];
        if (lm_gp) lm_gp[l] = P.lm_gp[l];
    }
    for (int b = 0; b < d.n_lblk && b < cap && lblk; ++b) {
        lblk[2 * b] = P.lblk_lm0[b];
        lblk[2 * b + 1] = P.lblk_n[b];
    }
    for (int b = 0; b < d.n_sblk && b < cap && sblk; ++b) {
        sblk[2 * b] = P.sblk_lm0[b];
        sblk[2 * b + 1] = P.sblk_n[b];
    }
    return LIMO_OK;
}

// 1 when the two packs of the windows - without a flags array, and with `lm_fixed` - give the same PackedBatch in every array and
// descriptor the kernels and the plan read: what "no change without flags" means for the packer.
int emu_pack_equal(int32_t n, const limo_ba_window* windows, const uint8_t* const* lm_fixed, const limo_ba_options* o) {
    PackedBatch A, B;
    std::string err;
    PackOptions pa, pb;
    pb.lm_fixed = lm_fixed;
    if (pack_windows(n, windows, *o, pa, A, err) != LIMO_OK || pack_windows(n, windows, *o, pb, B, err) != LIMO_OK) return -1;
    auto same = [](const auto& x, const auto& y) {
        return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0);
    };
    bool eq = A.n_win == B.n_win && A.TK == B.TK && A.TL == B.TL && A.TO == B.TO && A.TV == B.TV && A.TG == B.TG && A.n_blk == B.n_blk &&
              A.n_lblk == B.n_lblk && A.n_sblk == B.n_sblk && A.Vmax == B.Vmax && A.SO == B.SO && A.SL == B.SL && A.SG == B.SG &&
              A.hcc_total == B.hcc_total && A.spart_total == B.spart_total && A.camscr_total == B.camscr_total &&
              A.lvpart_total == B.lvpart_total && A.xlv_total == B.xlv_total;
    eq = eq && same(A.win, B.win) && same(A.pose, B.pose) && same(A.pdir, B.pdir) && same(A.pdist, B.pdist) && same(A.lm, B.lm) &&
         same(A.kf_win, B.kf_win) && same(A.kf_blk0, B.kf_blk0) && same(A.kf_nblk, B.kf_nblk) && same(A.kf_gp0, B.kf_gp0) &&
         same(A.kf_ngp, B.kf_ngp) && same(A.cmask, B.cmask) && same(A.cpresent, B.cpresent) && same(A.cslot, B.cslot) &&
         same(A.lm_gp, B.lm_gp) && same(A.lm_win, B.lm_win) && same(A.lm_slot, B.lm_slot) && same(A.lm_id, B.lm_id) &&
         same(A.lm_weight, B.lm_weight) && same(A.lm_state, B.lm_state) && same(A.view_kf, B.view_kf) && same(A.view_win, B.view_win) &&
         same(A.view_cam, B.view_cam) && same(A.blk_view, B.blk_view) && same(A.blk_obs0, B.blk_obs0) && same(A.blk_n, B.blk_n) &&
         same(A.obs_lm, B.obs_lm) && same(A.obs_u, B.obs_u) && same(A.obs_v, B.obs_v) && same(A.obs_d, B.obs_d) && same(A.obs_src, B.obs_src) &&
         same(A.lblk_win, B.lblk_win) && same(A.lblk_lm0, B.lblk_lm0) && same(A.lblk_n, B.lblk_n) && same(A.sblk_win, B.sblk_win) &&
         same(A.sblk_lm0, B.sblk_lm0) && same(A.sblk_n, B.sblk_n) && same(A.sgrp, B.sgrp) && same(A.gp_lm, B.gp_lm) && same(A.gp_kf, B.gp_kf) &&
         same(A.gp_w, B.gp_w);
    return eq ? 1 : 0;
}

}  // extern "C"
