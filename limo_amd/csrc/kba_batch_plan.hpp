// kba_batch_plan.hpp — what the host decides ONCE per batch from its packed layout: which Schur kernel variants serve it and how much
// dynamic LDS every kernel of the solve gets (BatchPlan), and the Schur worklists (build_sblk_list).  Host-only and free of the HIP
// runtime, so that the decisions are testable without a device (tests/cpp/test_batch_plan.cpp); limo_hip.hip turns the integers into
// kernel pointers.
#pragma once
#include <algorithm>
#include <cstdint>
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

}  // namespace kba
