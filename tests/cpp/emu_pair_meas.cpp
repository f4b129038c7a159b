// TEST INFRASTRUCTURE — the packer's pair-indexed measurement planes (kba_layout.hpp:BatchView::pair_m) next to the tables they are
// built from, for tests/test_pair_measurements_cpu.py.  The emulated pipeline is included as it stands (the buffers of an EmuBatch are
// what the kernels' BatchView points to).  Built by tests/pair_meas_common.py into tests/cpp/_build/libkba_emu_pairs.so.
#include "emu_pipeline.cpp"

extern "C" {

// Packs the windows (lm_fixed: NULL, or n entries, each NULL or that window's n_lm flags) and allocates the batch's buffers the way
// the library does (kba_buffers.hpp:for_each_buffer).  dims[6] = Vmax, SL, TL, TO, entries of lm_slot, entries of one plane of pair_m.  With
// slot != NULL the tables are copied out of the BATCH VIEW: slot / pu / pv / pd hold dims[4] entries, ou / ov / od dims[3], and
// win[4 * w] = lm0, n_lm, n_view, n_view_fixed0 of window w.
int emu_pair_planes(int32_t n, const limo_ba_window* windows, const uint8_t* const* lm_fixed, const limo_ba_options* o, int pose_only,
                    int64_t* dims, int32_t* slot, float* pu, float* pv, float* pd, float* ou, float* ov, float* od, int32_t* win) {
    EmuBatch B;
    std::string err;
    PackOptions po;
    po.lm_fixed = lm_fixed;
    po.pose_only = pose_only != 0;
    int rc = pack_windows(n, windows, *o, po, B.P, err);
    if (rc != LIMO_OK) return rc;
    const PackedBatch& P = B.P;
    dims[0] = P.Vmax, dims[1] = P.SL, dims[2] = P.TL, dims[3] = P.TO;
    dims[4] = (int64_t)P.lm_slot.size(), dims[5] = (int64_t)(P.pair_m.size() / 3);
    if (P.pair_m.size() % 3 != 0) return -100;
    if (!slot) return LIMO_OK;
    B.c = make_consts(*o);
    B.alloc();
    const BatchView& bv = B.bv;
    if (dims[4] != dims[5] || dims[4] != obs_c_stride(bv)) return -101;
    std::memcpy(slot, bv.lm_slot, sizeof(int32_t) * dims[4]);
    std::memcpy(pu, bv.pair_m, sizeof(float) * dims[4]);
    std::memcpy(pv, bv.pair_m + dims[4], sizeof(float) * dims[4]);
    std::memcpy(pd, bv.pair_m + 2 * dims[4], sizeof(float) * dims[4]);
    std::memcpy(ou, bv.obs_u, sizeof(float) * dims[3]);
    std::memcpy(ov, bv.obs_v, sizeof(float) * dims[3]);
    std::memcpy(od, bv.obs_d, sizeof(float) * dims[3]);
    for (int w = 0; w < n; ++w) {
        const WinDesc& d = P.win[w];
        win[4 * w] = d.lm0, win[4 * w + 1] = d.n_lm, win[4 * w + 2] = d.n_view, win[4 * w + 3] = d.n_view_fixed0;
    }
    return LIMO_OK;
}

}  // extern "C"
