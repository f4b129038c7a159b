// TEST — kba_items.hpp:cam_cov (the body of k_cam_cov) on three small hand-made camera systems, with no landmark and no Schur slab:
// the hand-over of cam_assemble is the whole system.  A stand-alone host program, built twice by tests/pose_cov_common.py: plain, and
// with -fsanitize=address,undefined (exact-size buffers: an index outside the window's scratch or matrix is an error there).
//   1. one keyframe, pose block only: cov = diag(s) S^-1 diag(s);
//   2. one keyframe with a free plane normal and distance: S = D J^T J D with the normal's columns of J projected by (I - n n^T) -
//      singular along n / scale; the pose block must equal that of the inverse in a minimal basis (two columns orthogonal to n);
//   3. two keyframes, the second one's pose block without any row: a zero pivot - LIMO_COV_RANK_DEFICIENT and NaN everywhere.
// Every case runs with one lane (the emulator's form of the statement); the lane-parallel form is the GPU tier's.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../limo_amd/csrc/kba_items.hpp"

using namespace kba;

namespace {

int g_fail = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
            ++g_fail;                                                           \
        }                                                                       \
    } while (0)

double rnd(unsigned& s) {  // (-1, 1)
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / (double)(1u << 23) - 1.0;
}

// Gauss-Jordan inverse with partial pivoting of a dense n x n matrix (row-major)
std::vector<double> inverse(std::vector<double> a, int n) {
    std::vector<double> b((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) b[(size_t)i * n + i] = 1.0;
    for (int k = 0; k < n; ++k) {
        int p = k;
        for (int i = k + 1; i < n; ++i)
            if (std::fabs(a[(size_t)i * n + k]) > std::fabs(a[(size_t)p * n + k])) p = i;
        for (int j = 0; j < n; ++j) {
            std::swap(a[(size_t)k * n + j], a[(size_t)p * n + j]);
            std::swap(b[(size_t)k * n + j], b[(size_t)p * n + j]);
        }
        const double d = a[(size_t)k * n + k];
        for (int j = 0; j < n; ++j) {
            a[(size_t)k * n + j] /= d;
            b[(size_t)k * n + j] /= d;
        }
        for (int i = 0; i < n; ++i) {
            if (i == k) continue;
            const double f = a[(size_t)i * n + k];
            for (int j = 0; j < n; ++j) {
                a[(size_t)i * n + j] -= f * a[(size_t)k * n + j];
                b[(size_t)i * n + j] -= f * b[(size_t)k * n + j];
            }
        }
    }
    return b;
}

// One window whose free slots are `free_slots` (local slot indices, ascending, pose slots of all keyframes first in the compact order)
struct Rig {
    WinDesc wd;
    WinRed red;
    BatchView bv;
    SolveConsts c;
    std::vector<uint8_t> cmask;
    std::vector<int32_t> cslot;
    std::vector<double> scale, pdir, Hcc, S_part, lblk_part, scratch, out;
    int32_t status = -1;

    Rig(int n_kf, const std::vector<int>& compact_to_slot, int nfq) {
        std::memset(&wd, 0, sizeof(wd));
        std::memset(&red, 0, sizeof(red));
        std::memset(&bv, 0, sizeof(bv));
        std::memset(&c, 0, sizeof(c));
        c.schur_span = 1;
        c.schur_span_gp = 1;
        const int nc = n_kf * kCamSlots, nf = (int)compact_to_slot.size();
        wd.n_kf = n_kf;
        wd.nc = nc;
        wd.nf = nf;
        wd.nfq = nfq;
        wd.nf_pad = (nf + 1 + 15) / 16 * 16;
        cmask.assign(nc, 0);
        cslot.assign(nc, -1);
        for (int i = 0; i < nf; ++i) {
            cmask[compact_to_slot[i]] = 1;
            cslot[compact_to_slot[i]] = i;
        }
        scale.assign(nc, 1.0);
        pdir.assign(3 * (size_t)n_kf, 0.0);
        Hcc.assign((size_t)schur_need_count(nf), 0.0);
        S_part.assign(1, 0.0);
        lblk_part.assign(8, 0.0);
        scratch.assign((size_t)cam_cov_scratch(nf, nfq), 0.0);
        out.assign((size_t)36 * n_kf * n_kf, -7.0);
        bv.n_win = 1;
        bv.win = &wd;
        bv.red = &red;
        bv.cmask = cmask.data();
        bv.cslot = cslot.data();
        bv.scale_c = scale.data();
        bv.pdir = pdir.data();
        bv.Hcc = Hcc.data();
        bv.S_part = S_part.data();
        bv.lblk_part = lblk_part.data();
    }
    // the hand-over: upper triangle of the scaled system S (compact order, nf x nf row-major), rhs entries zero
    void hand_over(const std::vector<double>& S) {
        const int nf = wd.nf;
        for (int i = 0; i < schur_need_count(nf); ++i) {
            int ca, cb;
            schur_need_decode(i, nf, ca, cb);
            Hcc[i] = cb < nf ? S[(size_t)ca * nf + cb] : 0.0;
        }
    }
    void run() { cam_cov(bv, c, 0, 0, 1, scratch.data(), out.data(), &status); }
};

double rel_frob(const std::vector<double>& got, const std::vector<double>& want) {
    double num = 0.0, den = 0.0;
    for (size_t i = 0; i < want.size(); ++i) {
        num += (got[i] - want[i]) * (got[i] - want[i]);
        den += want[i] * want[i];
    }
    return std::sqrt(num / den);
}

void check_symmetric_positive(const Rig& r, int n6) {
    for (int i = 0; i < n6; ++i)
        for (int j = 0; j < n6; ++j) CHECK(std::memcmp(&r.out[(size_t)i * n6 + j], &r.out[(size_t)j * n6 + i], sizeof(double)) == 0);
}

void case_pose_only() {
    unsigned seed = 11;
    const int nf = 6, m = 14;
    Rig r(1, {0, 1, 2, 3, 4, 5}, 6);
    std::vector<double> J((size_t)m * nf), S((size_t)nf * nf, 0.0), U((size_t)nf * nf, 0.0);
    for (double& v : J) v = rnd(seed);
    for (int i = 0; i < nf; ++i) r.scale[i] = 0.3 + 0.1 * i;
    for (int a = 0; a < nf; ++a)
        for (int b = 0; b < nf; ++b) {
            double s = 0.0;
            for (int k = 0; k < m; ++k) s += J[(size_t)k * nf + a] * J[(size_t)k * nf + b];
            U[(size_t)a * nf + b] = s;
            S[(size_t)a * nf + b] = r.scale[a] * s * r.scale[b];
        }
    r.hand_over(S);
    r.run();
    CHECK(r.status == LIMO_COV_OK);
    const std::vector<double> want = inverse(U, nf);
    const double e = rel_frob(r.out, want);
    std::printf("pose block only: relative error %.2e\n", e);
    CHECK(e < 1e-12);
    check_symmetric_positive(r, 6);
    for (int i = 0; i < 6; ++i) CHECK(r.out[(size_t)i * 6 + i] > 0.0);
}

void case_free_normal() {
    unsigned seed = 23;
    const int nf = 10, m = 24;
    std::vector<int> slots(nf);
    for (int i = 0; i < nf; ++i) slots[i] = i;
    Rig r(1, slots, 6);
    double n[3] = {0.2, -0.9, 0.3};
    const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (double& v : n) v /= len;
    for (int i = 0; i < 3; ++i) r.pdir[i] = n[i];
    std::vector<double> J((size_t)m * nf);
    for (double& v : J) v = rnd(seed);
    for (int k = 0; k < m; ++k) {  // the normal's columns 6..8: J_n (I - n n^T)
        double* row = J.data() + (size_t)k * nf + 6;
        const double d = row[0] * n[0] + row[1] * n[1] + row[2] * n[2];
        for (int i = 0; i < 3; ++i) row[i] -= d * n[i];
    }
    for (int i = 0; i < nf; ++i) r.scale[i] = 0.2 + 0.07 * i;
    std::vector<double> S((size_t)nf * nf, 0.0);
    for (int a = 0; a < nf; ++a)
        for (int b = 0; b < nf; ++b) {
            double s = 0.0;
            for (int k = 0; k < m; ++k) s += J[(size_t)k * nf + a] * J[(size_t)k * nf + b];
            S[(size_t)a * nf + b] = r.scale[a] * s * r.scale[b];
        }
    r.hand_over(S);
    r.run();
    CHECK(r.status == LIMO_COV_OK);
    // minimal basis: two unit columns orthogonal to n
    double b1[3], b2[3];
    {
        const double t[3] = {1.0, 0.0, 0.0};
        const double d = t[0] * n[0] + t[1] * n[1] + t[2] * n[2];
        double l = 0.0;
        for (int i = 0; i < 3; ++i) {
            b1[i] = t[i] - d * n[i];
            l += b1[i] * b1[i];
        }
        for (double& v : b1) v /= std::sqrt(l);
        b2[0] = n[1] * b1[2] - n[2] * b1[1];
        b2[1] = n[2] * b1[0] - n[0] * b1[2];
        b2[2] = n[0] * b1[1] - n[1] * b1[0];
    }
    const int nm = 9;
    std::vector<double> Jm((size_t)m * nm);
    for (int k = 0; k < m; ++k) {
        const double* row = J.data() + (size_t)k * nf;
        double* o = Jm.data() + (size_t)k * nm;
        for (int i = 0; i < 6; ++i) o[i] = row[i];
        o[6] = row[6] * b1[0] + row[7] * b1[1] + row[8] * b1[2];
        o[7] = row[6] * b2[0] + row[7] * b2[1] + row[8] * b2[2];
        o[8] = row[9];
    }
    std::vector<double> N((size_t)nm * nm, 0.0);
    for (int a = 0; a < nm; ++a)
        for (int b = 0; b < nm; ++b)
            for (int k = 0; k < m; ++k) N[(size_t)a * nm + b] += Jm[(size_t)k * nm + a] * Jm[(size_t)k * nm + b];
    const std::vector<double> Ni = inverse(N, nm);
    std::vector<double> want(36);
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) want[(size_t)a * 6 + b] = Ni[(size_t)a * nm + b];
    const double e = rel_frob(r.out, want);
    std::printf("free plane normal: relative error %.2e\n", e);
    CHECK(e < 1e-11);
    check_symmetric_positive(r, 6);
}

void case_zero_pivot() {
    unsigned seed = 5;
    // two keyframes, pose blocks free: compact 0..5 = slots 0..5, compact 6..11 = slots 10..15; nothing constrains the second one
    std::vector<int> slots;
    for (int i = 0; i < 6; ++i) slots.push_back(i);
    for (int i = 0; i < 6; ++i) slots.push_back(kCamSlots + i);
    const int nf = 12, m = 14;
    Rig r(2, slots, 12);
    std::vector<double> J((size_t)m * 6), S((size_t)nf * nf, 0.0);
    for (double& v : J) v = rnd(seed);
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b)
            for (int k = 0; k < m; ++k) S[(size_t)a * nf + b] += J[(size_t)k * 6 + a] * J[(size_t)k * 6 + b];
    r.hand_over(S);
    r.run();
    CHECK(r.status == LIMO_COV_RANK_DEFICIENT);
    for (double v : r.out) CHECK(std::isnan(v));
    // ... and with a pivot that is tiny but not zero: 1e-9 of its diagonal entry is below 2^-26
    for (int a = 6; a < 12; ++a) S[(size_t)a * nf + a] = 1.0;
    S[(size_t)6 * nf + 7] = S[(size_t)7 * nf + 6] = 1.0 - 1e-9;
    Rig q(2, slots, 12);
    q.hand_over(S);
    q.run();
    CHECK(q.status == LIMO_COV_RANK_DEFICIENT);
    // a window without a free pose block: zeros
    Rig z(1, {6, 7, 8, 9}, 0);
    z.run();
    CHECK(z.status == LIMO_COV_NO_FREE_POSE);
    for (double v : z.out) CHECK(v == 0.0);
    // a failed linearisation: NaN
    Rig f(1, {0, 1, 2, 3, 4, 5}, 6);
    f.red.lin_fail = 1;
    f.run();
    CHECK(f.status == LIMO_COV_EVAL_FAILED);
    for (double v : f.out) CHECK(std::isnan(v));
}

}  // namespace

int main() {
    case_pose_only();
    case_free_normal();
    case_zero_pivot();
    std::printf(g_fail ? "%d checks FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
