// Host-only check of the class of ground-plane Schur groups (kba_layout.hpp:SchurGroup::gp_class, written by
// kba_items.hpp:schur_group_make from the row tables lm_gp / gp_kf) and of the column map of the narrow tile (schur_narrow_col /
// schur_narrow_zc / schur_narrow_covers).  Stand-alone program, built with -fsanitize=address,undefined by
// tests/test_schur_narrow_cpu.py.  The windows are written out by hand (which keyframe a landmark's row hangs on is an input
// here), and so are the expected classes.  The batch-level rule - groups are classified only where the batch's ground-plane tile has
// three panels - is schur_gp_panels, checked at the end; what a packed batch then counts is checked on the GPU tier.
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
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

// A window of 5 keyframes (keyframe 0 Pose-fixed: no free slot at all; keyframes 1 .. 4 free, 4 plane slots each unless
// `planes3`: then slot 9 is fixed everywhere) from global keyframe 20, landmarks from 500: n_plain plain landmarks, then n_gp with
// a ground-plane row, then n_const constant ones (no Schur block).  row_kf[i] = local keyframe of the row of ground-plane landmark i.
struct Hand {
    WinDesc d;
    std::vector<int32_t> sblk_lm0, sblk_n, cslot, lm_gp, gp_kf;
};
static Hand make(int n_plain, const std::vector<int>& row_kf, int n_const, bool planes3, int fixed_kf = -1) {
    Hand h;
    WinDesc& d = h.d;
    std::memset(&d, 0, sizeof(d));
    const int n_gp = (int)row_kf.size();
    d.kf0 = 20, d.n_kf = 5, d.cam0 = 200, d.view0 = 3, d.n_view = 5;
    d.lm0 = 500, d.n_lm = n_plain + n_gp + n_const, d.lm_gp0 = 500 + n_plain, d.n_lm_const = n_const;
    d.schur_fast = 1, d.n_fk = 0;
    h.cslot.assign(250, -1);
    int nf = 0;
    for (int pass = 0; pass < 2; ++pass) {  // compact numbering as kba_pack.cpp gives it: pose slots first, then plane slots
        for (int k = 1; k < 5; ++k) {
            if (k == fixed_kf) continue;
            for (int s = pass ? 6 : 0; s < (pass ? (planes3 ? 9 : 10) : 6); ++s) h.cslot[200 + 10 * k + s] = nf++;
        }
        if (pass == 0) d.nfq = nf;
    }
    d.nf = nf, d.nf_pad = (nf + 1 + 15) / 16 * 16;
    for (int k = 1; k < 5; ++k)
        if (k != fixed_kf) d.fk[d.n_fk] = k, d.fk_view[d.n_fk] = 3 + k, d.n_fk++;
    d.sblk0 = 7;
    h.sblk_lm0.assign(7, -9), h.sblk_n.assign(7, -9);
    for (int l0 = 0; l0 < n_plain; l0 += 64) h.sblk_lm0.push_back(500 + l0), h.sblk_n.push_back(std::min(64, n_plain - l0)), d.n_sblk_plain++;
    for (int l0 = 0; l0 < n_gp; l0 += 64) h.sblk_lm0.push_back(500 + n_plain + l0), h.sblk_n.push_back(std::min(64, n_gp - l0));
    d.n_sblk = (int)h.sblk_lm0.size() - 7;
    // rows sorted by keyframe (stable), as the pack lays them out; global row indices from 40
    h.lm_gp.assign(500 + d.n_lm, -1);
    h.gp_kf.assign(40, -1);
    for (int k = 0; k < 5; ++k)
        for (int i = 0; i < n_gp; ++i)
            if (row_kf[i] == k) {
                h.lm_gp[500 + n_plain + i] = (int)h.gp_kf.size();
                h.gp_kf.push_back(20 + k);
            }
    return h;
}
static SchurGroup group(const Hand& h, int gp_block, bool tables = true, int span_gp = 1) {
    return schur_group_make(h.d, 0, h.d.sblk0 + h.d.n_sblk_plain + gp_block, 2, span_gp, h.sblk_lm0.data(), h.sblk_n.data(), h.cslot.data(),
                            tables ? h.lm_gp.data() : nullptr, tables ? h.gp_kf.data() : nullptr);
}

// The column map of a record against the slab entries the camera solve reads (slab_packed_read(true, ca, cb), ca <= cb <= nf):
// every entry is either covered by exactly one upper-triangle entry of the narrow tile, which maps to it, or by none - then it
// involves a plane slot outside the tile - and the covered ones are exactly the pairs of covered slots.
static void check_map(const SchurGroup& g) {
    const int nf = g.nf, nfq = g.nfq, ci0 = g.gp_ci0, ns = g.gp_ns, ncol = nfq + 1 + ns;
    CHECK(ncol <= 32);
    std::vector<int> hits(schur_need_count(nf), 0);
    for (int r = 0; r < ncol; ++r)
        for (int c = r; c < ncol; ++c) {
            const int zr = schur_narrow_zc(r, nfq, ci0), zc = schur_narrow_zc(c, nfq, ci0);
            CHECK(schur_narrow_col(zr, nfq, ci0, ns) == r && schur_narrow_col(zc, nfq, ci0, ns) == c);
            const int k = slab_packed_write(true, zr, zc, nf, nfq);
            if (r == nfq && c == nfq) {
                CHECK(k == -1);  // |t|^2: nobody reads it
                continue;
            }
            CHECK(k >= 0 && k < (int)hits.size());
            if (k >= 0 && k < (int)hits.size()) hits[k]++;
        }
    int uncovered = 0;
    for (int ca = 0; ca < nf; ++ca)
        for (int cb = ca; cb <= nf; ++cb) {
            const int k = slab_packed_read(true, ca, cb, nf, nfq);
            const bool cov = schur_narrow_covers(ca, nfq, ci0, ns) && (cb == nf || schur_narrow_covers(cb, nfq, ci0, ns));
            CHECK(hits[k] == (cov ? 1 : 0));
            uncovered += cov ? 0 : 1;
            // what the epilogue of the narrow wave zero-fills: column cb in [nfq, nf], a slot of the pair outside the tile
            if (!cov) CHECK(cb >= nfq && (ca >= nfq || cb < nf));
        }
    const int nu = nf - nfq - ns;  // plane slots without a column
    CHECK(uncovered == schur_need_count(nf) - (schur_need_count(nfq + ns)));
    CHECK(nu >= 0);
    for (int zc = 0; zc <= nf; ++zc)  // columns outside the tile map to -1
        if (zc > nfq && !(zc - 1 >= ci0 && zc - 1 < ci0 + ns)) CHECK(schur_narrow_col(zc, nfq, ci0, ns) == -1);
}

int main() {
    {   // all rows on the newest keyframe: 100 ground-plane landmarks, blocks of 64 + 36
        const Hand h = make(150, std::vector<int>(100, 4), 0, false);
        CHECK(h.d.nfq == 24 && h.d.nf == 40 && h.d.n_sblk == 5 && h.d.n_sblk_plain == 3);
        for (int b = 0; b < 2; ++b) {
            const SchurGroup g = group(h, b);
            CHECK(g.gp_class == 4 && g.gp_ci0 == 36 && g.gp_ns == 4 && g.n_lm == (b ? 36 : 64));
            check_map(g);
        }
        CHECK(group(h, 0, false).gp_class == kSchurGpWide);  // the device route: no tables
        // a plain group has no class
        CHECK(schur_group_make(h.d, 0, h.d.sblk0, 2, 1, h.sblk_lm0.data(), h.sblk_n.data(), h.cslot.data(), h.lm_gp.data(), h.gp_kf.data()).gp_class == kSchurGpWide);
    }
    {   // rows on two keyframes inside one block of 64: wide; the second block (all on keyframe 3) narrow, three plane slots per keyframe
        std::vector<int> kf(70, 3);
        kf[10] = 2;
        const Hand h = make(64, kf, 0, true);
        CHECK(h.d.nfq == 24 && h.d.nf == 36);
        const SchurGroup g0 = group(h, 0), g1 = group(h, 1);
        CHECK(g0.gp_class == kSchurGpWide && g0.gp_ci0 == 0 && g0.gp_ns == 0);
        CHECK(g1.gp_class == 3 && g1.gp_ci0 == 24 + 3 * 2 && g1.gp_ns == 3 && g1.n_lm == 6);  // a last block of 6 landmarks
        check_map(g1);
        // one group over both blocks (span 2): wide
        CHECK(group(h, 0, true, 2).gp_class == kSchurGpWide && group(h, 0, true, 2).n_lm == 70);
    }
    {   // the same two keyframes in different blocks: both narrow, each on its keyframe - a tile whose plane columns sit in the
        // middle of the plane range
        std::vector<int> kf(70, 2);
        for (int i = 64; i < 70; ++i) kf[i] = 3;
        const Hand h = make(10, kf, 0, false);
        const SchurGroup g0 = group(h, 0), g1 = group(h, 1);
        CHECK(g0.gp_class == 2 && g0.gp_ci0 == 28 && g0.gp_ns == 4);
        CHECK(g1.gp_class == 3 && g1.gp_ci0 == 32 && g1.gp_ns == 4);
        check_map(g0);
        check_map(g1);
    }
    {   // rows only on a keyframe with no free plane slot (keyframe 4 Pose-fixed): narrow without plane columns; with one
        // landmark on a free keyframe besides: narrow on that one; rows on keyframe 0 (no slot at all) count like keyframe 4's
        std::vector<int> kf(40, 4);
        const Hand h = make(64, kf, 0, false, 4);
        CHECK(h.d.nfq == 18 && h.d.nf == 30 && h.d.n_fk == 3);
        const SchurGroup g = group(h, 0);
        CHECK(g.gp_class == kSchurGpNoPlane && g.gp_ci0 == 0 && g.gp_ns == 0);
        check_map(g);
        kf[7] = 1, kf[8] = 0;
        const Hand h2 = make(64, kf, 0, false, 4);
        const SchurGroup g2 = group(h2, 0);
        CHECK(g2.gp_class == 1 && g2.gp_ci0 == 18 && g2.gp_ns == 4);
        check_map(g2);
        kf[9] = 2;
        CHECK(group(make(64, kf, 0, false, 4), 0).gp_class == kSchurGpWide);
    }
    {   // constant landmarks behind the ground-plane run (their rows hang on another keyframe): not part of any group
        const Hand h0 = make(30, std::vector<int>(20, 4), 0, false);
        Hand h = make(30, std::vector<int>(20, 4), 12, false);
        for (int i = 0; i < 12; ++i) {  // rows of the constant landmarks, on keyframe 1
            h.lm_gp[500 + 50 + i] = (int)h.gp_kf.size();
            h.gp_kf.push_back(21);
        }
        const SchurGroup g = group(h, 0);
        CHECK(h.d.n_sblk == h0.d.n_sblk && g.n_lm == 20 && g.gp_class == 4);
    }
    {   // free plane slots behind a fixed pose block (no packed window has them): left to the wide tile
        Hand h = make(10, std::vector<int>(20, 4), 0, false);
        for (int s = 0; s < 6; ++s) h.cslot[200 + 40 + s] = -1;
        CHECK(group(h, 0).gp_class == kSchurGpWide);
    }
    {   // panels of the batch's ground-plane tile: 2 and 3 free keyframes (nf + 1 = 21, 31 columns) give two - nothing is classified -,
        // four give three; windows outside the fast class do not count
        std::vector<WinDesc> win(3);
        std::memset(win.data(), 0, sizeof(WinDesc) * win.size());
        win[0].schur_fast = 1, win[0].nf = 20;
        win[1].schur_fast = 1, win[1].nf = 30;
        win[2].schur_fast = 0, win[2].nf = 90;
        CHECK(schur_gp_panels(win) == 2);
        win[1].nf = 31;
        CHECK(schur_gp_panels(win) == 2);
        win[1].nf = 32;
        CHECK(schur_gp_panels(win) == 3);
        win[1].nf = 40;
        CHECK(schur_gp_panels(win) == 3);
        win[0].nf = win[1].nf = 10;
        CHECK(schur_gp_panels(win) == 1);
    }
    CHECK(sizeof(SchurGroup) == 128);
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
