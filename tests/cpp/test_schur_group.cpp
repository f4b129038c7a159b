// Host-only check of the Schur group record (kba_layout.hpp:SchurGroup, kba_items.hpp:schur_group_make): what a lean Schur wave
// knows about its group before its first load.  Stand-alone program, built with -fsanitize=address by tests/test_schur_group_cpu.py.
// The expected values are written out here from the window's layout (landmarks of a class are contiguous, 64 per block), not computed
// by the code under test.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../limo_amd/csrc/kba_items.hpp"

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

int main() {
    // Window 3 of a batch: 4 keyframes from global keyframe 12 (camera slots from 120), views from 9, landmarks from 1000:
    // 150 plain landmarks (blocks of 64, 64, 22) and 70 with a ground-plane row (blocks of 64, 6); Schur blocks from 40.
    // Keyframe 0 is Pose-fixed (only its plane slots are free), keyframes 1 .. 3 are free; keyframe 2 has NO view.
    WinDesc d;
    std::memset(&d, 0, sizeof(d));
    d.kf0 = 12, d.n_kf = 4, d.cam0 = 120, d.view0 = 9, d.n_view = 3;
    d.lm0 = 1000, d.n_lm = 220, d.lm_gp0 = 1150;
    d.sblk0 = 40, d.n_sblk = 5, d.n_sblk_plain = 3;
    d.schur_fast = 1, d.n_fk = 4;
    const int fk[4] = {0, 1, 2, 3}, fk_view[4] = {9, 10, -1, 11};
    for (int k = 0; k < 4; ++k) d.fk[k] = fk[k], d.fk_view[k] = fk_view[k];
    d.nfq = 18, d.nf = 34, d.nf_pad = 48;  // 3 free pose blocks, 4 x 4 plane slots
    d.spart_off = 100000;
    std::vector<int32_t> sblk_lm0(45, -7), sblk_n(45, -7), cslot(160, -1);
    const int lm0s[5] = {1000, 1064, 1128, 1150, 1214}, ns[5] = {64, 64, 22, 64, 6};
    for (int i = 0; i < 5; ++i) sblk_lm0[40 + i] = lm0s[i], sblk_n[40 + i] = ns[i];
    // compact numbering: pose slots of keyframes 1, 2, 3 first (0 .. 17), then the plane slots of keyframes 0 .. 3 (18 .. 33)
    for (int k = 1; k < 4; ++k)
        for (int i = 0; i < 6; ++i) cslot[120 + 10 * k + i] = 6 * (k - 1) + i;
    for (int k = 0; k < 4; ++k)
        for (int i = 6; i < 10; ++i) cslot[120 + 10 * k + i] = 18 + 4 * k + (i - 6);

    struct Want {
        int sb, span, span_gp, lm_first, n_lm, q_slab;
        long long off_tile, off_packed;
    };
    const long long pl = schur_need_pad(18), gp = schur_need_pad(34);  // strides of the packed slabs (their sizes are checked elsewhere)
    const Want want[] = {
        // spans 2 / 1: plain groups {40, 41}, {42}; ground-plane groups {43}, {44}; two plain slabs
        {40, 2, 1, 1000, 128, 0, 100000, 100000},
        {42, 2, 1, 1128, 22, 1, 100000 + 48 * 48, 100000 + pl},
        {43, 2, 1, 1150, 64, 2, 100000 + 2 * 48 * 48, 100000 + 2 * pl},
        {44, 2, 1, 1214, 6, 3, 100000 + 3 * 48 * 48, 100000 + 2 * pl + gp},
        // spans 1 / 1: one block per group; three plain slabs
        {41, 1, 1, 1064, 64, 1, 100000 + 48 * 48, 100000 + pl},
        {42, 1, 1, 1128, 22, 2, 100000 + 2 * 48 * 48, 100000 + 2 * pl},
        {44, 1, 1, 1214, 6, 4, 100000 + 4 * 48 * 48, 100000 + 3 * pl + gp},
    };
    for (const Want& x : want) {
        const SchurGroup g = schur_group_make(d, 3, x.sb, x.span, x.span_gp, sblk_lm0.data(), sblk_n.data(), cslot.data());
        CHECK(g.w == 3 && g.lm_first == x.lm_first && g.n_lm == x.n_lm && g.q_slab == x.q_slab);
        CHECK(g.off_tile == x.off_tile && g.off_packed == x.off_packed);
        CHECK(g.n_fk == 4 && g.nf == 34 && g.nfq == 18 && g.nf_pad == 48 && g.kf0 == 12 && g.view0 == 9 && g.cam0 == 120);
        CHECK(g.kl[0] == 0 && g.kl[1] == 1 && g.kl[2] == 2 && g.kl[3] == 3);
        CHECK(g.view[0] == 9 && g.view[1] == 10 && g.view[2] == -1 && g.view[3] == 11);
        // keyframe 0: pose block not free; keyframe 2: free WITHOUT a view - column of its first pose slot, view -1
        CHECK(g.col0[0] == -1 && g.col0[1] == 0 && g.col0[2] == 6 && g.col0[3] == 12);
    }
    {   // fewer free keyframes than four: the idle entries are -1 throughout
        WinDesc e = d;
        e.n_fk = 2;
        const SchurGroup g = schur_group_make(e, 0, 40, 2, 1, sblk_lm0.data(), sblk_n.data(), cslot.data());
        CHECK(g.n_fk == 2 && g.kl[2] == -1 && g.kl[3] == -1 && g.view[2] == -1 && g.view[3] == -1 && g.col0[2] == -1 && g.col0[3] == -1);
        CHECK(g.kl[1] == 1 && g.view[1] == 10 && g.col0[1] == 0);
    }
    CHECK(sizeof(SchurGroup) == 128 && alignof(SchurGroup) == 128);
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
