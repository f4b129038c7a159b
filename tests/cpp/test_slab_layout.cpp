// TEST INFRASTRUCTURE - the index helpers of the packed Schur partial slabs (limo_amd/csrc/kba_items.hpp: slab_packed_write,
// slab_packed_read, slab_packed_base) on the host: for every system size that occurs (nf <= 40 free slots, of which nfq pose
// slots in blocks of 6 and nf - nfq plane slots in blocks of 4) the writer map (tile row, tile column in schur_col space) and
// the reader map (ca, cb of cam_solve's enumeration) must name the same places, every place exactly once, inside the slab.
#include <cstdio>
#include <vector>

#include "../../limo_amd/csrc/kba_items.hpp"

using namespace kba;

static int n_fail = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (++n_fail <= 20) {                 \
                std::printf("FAILED %s: ", #cond); \
                std::printf(__VA_ARGS__);         \
                std::printf("\n");                \
            }                                     \
        }                                         \
    } while (0)

static void check_system(int nf, int nfq) {
    const int nfp = (nf + 1 + 15) / 16 * 16;
    for (int gp = 0; gp < 2; ++gp) {
        const int n = gp ? nf : nfq;  // slots of a slab of the class
        const int count = schur_need_count(n), stride = schur_need_pad(n);
        CHECK(count <= stride && stride % 32 == 0 && stride <= nfp * nfp, "nf %d nfq %d gp %d", nf, nfq, gp);
        // writer: every entry of the padded tile matrix - each packed place is written from exactly one of them
        std::vector<int> hits(stride, 0);
        for (int zr = 0; zr < nfp; ++zr)
            for (int zc = 0; zc < nfp; ++zc) {
                const int k = slab_packed_write(gp != 0, zr, zc, nf, nfq);
                CHECK(k >= -1 && k < count, "nf %d nfq %d gp %d (%d, %d) -> %d", nf, nfq, gp, zr, zc, k);
                if (k >= 0 && k < stride) ++hits[k];
                // nobody reads the lower triangle, |t|^2, the padding, and - plain slab - anything that involves a plane column
                if (zr > zc || zc > nf || (zr == nfq && zc == nfq) || (!gp && zc > nfq)) CHECK(k == -1, "nf %d nfq %d gp %d (%d, %d) -> %d", nf, nfq, gp, zr, zc, k);
            }
        for (int k = 0; k < stride; ++k) CHECK(hits[k] == (k < count ? 1 : 0), "nf %d nfq %d gp %d: place %d written %d times", nf, nfq, gp, k, hits[k]);
        // reader: cam_solve's enumeration for nf; the entry's tile position is where the tile-layout reader finds it
        std::vector<int> read(stride, 0);
        for (int i = 0; i < schur_need_count(nf); ++i) {
            int ca, cb;
            schur_need_decode(i, nf, ca, cb);
            const int64_t off = schur_need_offset(ca, cb, nf, nfq, nfp);
            const int zr = (int)(off / nfp), zc = (int)(off % nfp);
            const int r = slab_packed_read(gp != 0, ca, cb, nf, nfq), wr = slab_packed_write(gp != 0, zr, zc, nf, nfq);
            CHECK(r == wr, "nf %d nfq %d gp %d entry %d (%d, %d): reader %d, writer %d", nf, nfq, gp, i, ca, cb, r, wr);
            const bool plane = ca >= nfq || (cb >= nfq && cb < nf);
            if (gp) CHECK(r == i, "nf %d nfq %d entry %d -> %d", nf, nfq, i, r);  // the order S_red keeps under schur_packed
            if (!gp) CHECK((r == -1) == plane, "nf %d nfq %d entry %d (%d, %d) -> %d", nf, nfq, i, ca, cb, r);
            CHECK(r >= -1 && r < count && r < stride, "nf %d nfq %d gp %d entry %d -> %d", nf, nfq, gp, i, r);
            if (r >= 0 && r < stride) ++read[r];
        }
        for (int k = 0; k < stride; ++k) CHECK(read[k] == (k < count ? 1 : 0), "nf %d nfq %d gp %d: place %d read %d times", nf, nfq, gp, k, read[k]);
    }
    // the two-tile epilogue of the plain Schur wave (kba_kernels.hip:schur_lean_group, 17 .. 25 tile columns): lane (kq, li),
    // register r holds entry (kq + 4 r, 8 + li) of the first product and (m(kq + 4 r), m(li)) of the second, m = {0..7, 16..23};
    // the rhs of slot s is entry (s, nfq).  Together: every place of a plain slab once.
    if (nfq + 1 > 16 && nfq <= 24) {
        std::vector<int> hits(schur_need_pad(nfq), 0);
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) {
                const int li = lane & 15, kq = lane >> 4, row = kq + 4 * r, mq = li < 8 ? li : li + 8;
                if (row <= 8 + li && 8 + li < nfq) ++hits[slab_packed_write(false, row, 8 + li, nf, nfq)];
                const int a = row < 8 ? row : row + 8;
                if (a <= mq && mq < nfq && !(a < 8 && mq >= 16)) ++hits[slab_packed_write(false, a, mq, nf, nfq)];
            }
        for (int s = 0; s < nfq; ++s) ++hits[slab_packed_write(false, s, nfq, nf, nfq)];
        for (int k = 0; k < schur_need_pad(nfq); ++k) CHECK(hits[k] == (k < schur_need_count(nfq) ? 1 : 0), "two-tile nf %d nfq %d: place %d written %d times", nf, nfq, k, hits[k]);
    }
    // the slabs of a window lie back to back, in slab order, inside the region the tile layout is allotted (one nfp x nfp
    // matrix per Schur block; a plain slab takes up to `span` = 2 blocks, a ground-plane slab one)
    for (int n_plain_blk = 0; n_plain_blk <= 9; ++n_plain_blk)
        for (int n_gp_blk = 0; n_gp_blk <= 5; ++n_gp_blk) {
            const int P = (n_plain_blk + 1) / 2, n_slab = P + n_gp_blk;
            int64_t end = 0;
            for (int q = 0; q < n_slab; ++q) {
                const int64_t b = slab_packed_base(q, P, nf, nfq);
                CHECK(b == end, "nf %d nfq %d P %d slab %d starts at %lld, the one before ends at %lld", nf, nfq, P, q, (long long)b, (long long)end);
                end = b + schur_need_pad(q < P ? nfq : nf);
            }
            CHECK(end <= (int64_t)(n_plain_blk + n_gp_blk) * nfp * nfp, "nf %d nfq %d: %d + %d blocks", nf, nfq, n_plain_blk, n_gp_blk);
            // cam_solve's load of a skipped term (an entry index of the nf system from the last ground-plane slab's start, or
            // from the region's start when there is none) stays inside the region
            if (n_slab > 0) {
                const int64_t skip = n_slab > P ? slab_packed_base(n_slab - 1, P, nf, nfq) : 0;
                CHECK(skip + schur_need_count(nf) <= (int64_t)(n_plain_blk + n_gp_blk) * nfp * nfp, "nf %d nfq %d: %d + %d blocks", nf, nfq, n_plain_blk, n_gp_blk);
            }
        }
}

int main() {
    int n_sys = 0;
    for (int nf = 0; nf <= 40; ++nf)
        for (int nfq = 0; nfq <= nf; nfq += 6)
            if ((nf - nfq) % 4 == 0) {
                check_system(nf, nfq);
                ++n_sys;
            }
    std::printf("%d systems, %d failed checks\n", n_sys, n_fail);
    return n_fail ? 1 : 0;
}
