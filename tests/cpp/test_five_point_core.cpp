// test_five_point_core.cpp — limo_amd/csrc/five_point_core.hpp (the statement the device runs) against limo_amd/kba/five_point.hpp
// (the host estimator), bit for bit.  A stand-alone host program: built plainly and under -fsanitize=address,undefined by
// tests/five_point_common.py, run by tests/test_five_point_core_cpu.py.
//   1. fp5::essential_from_five against five_point::essentialFromFive: same number of models, same order, same bits, over random
//      minimal samples (clean, noisy, random) and degenerate ones.
//   2. the chunked pipeline as limo_five_point runs it - all samples of a chunk, FULL inlier counts, then the stopping rule over the
//      counts (fp5::scan_chunk), mask and pose of the winner - against five_point::estimateMotion: the whole Motion and the mask.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../limo_amd/csrc/five_point_core.hpp"
#include "../../limo_amd/kba/five_point.hpp"

namespace kb = keyframe_bundle_adjustment;
namespace fp5 = kba::fp5;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            if (++g_fail <= 20) {                                \
                std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                        \
                std::printf("\n");                               \
            }                                                    \
        }                                                        \
    } while (0)

static bool same_bits(const double* a, const double* b, int n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

// ---- scenes: points in front of a camera that moves forward and turns a little; a = first view, b = second, normalised coordinates
struct Scene {
    double R[9], t[3];
};
static Scene make_motion(std::mt19937_64& rng, bool pure_rotation) {
    std::uniform_real_distribution<double> U(-1., 1.);
    Scene s;
    const double yaw = 0.05 * U(rng), pitch = 0.01 * U(rng);
    const double cy = std::cos(yaw), sy = std::sin(yaw), cp = std::cos(pitch), sp = std::sin(pitch);
    const double Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s.R[3 * i + j] = Ry[3 * i] * Rx[j] + Ry[3 * i + 1] * Rx[3 + j] + Ry[3 * i + 2] * Rx[6 + j];
    s.t[0] = pure_rotation ? 0. : 0.1 * U(rng);
    s.t[1] = pure_rotation ? 0. : 0.02 * U(rng);
    s.t[2] = pure_rotation ? 0. : -1.;
    return s;
}
static void project(const Scene& s, const double X[3], double a[2], double b[2]) {
    a[0] = X[0] / X[2];
    a[1] = X[1] / X[2];
    const double Y[3] = {s.R[0] * X[0] + s.R[1] * X[1] + s.R[2] * X[2] + s.t[0], s.R[3] * X[0] + s.R[4] * X[1] + s.R[5] * X[2] + s.t[1],
                         s.R[6] * X[0] + s.R[7] * X[1] + s.R[8] * X[2] + s.t[2]};
    b[0] = Y[0] / Y[2];
    b[1] = Y[1] / Y[2];
}

// ---- 1. the minimal solver
struct SolverStats {
    int samples = 0, zero = 0, four_or_more = 0, models = 0;
};
static void check_sample(const double a[5][2], const double b[5][2], SolverStats& st, const char* what) {
    const std::vector<kb::five_point::Mat3> want = kb::five_point::essentialFromFive(a, b);
    double ws[fp5::kWs], out[9 * fp5::kMaxModels];
    const int got = fp5::essential_from_five(&a[0][0], &b[0][0], ws, out);
    CHECK(got == (int)want.size(), "%s sample %d: %d models, the host has %zu", what, st.samples, got, want.size());
    for (int k = 0; k < got && k < (int)want.size(); ++k)
        CHECK(same_bits(out + 9 * k, want[k].data(), 9), "%s sample %d model %d: bits differ (%.17g vs %.17g)", what, st.samples, k, out[9 * k], want[k][0]);
    ++st.samples;
    st.zero += want.empty();
    st.four_or_more += want.size() >= 4;
    st.models += (int)want.size();
}

static void test_minimal_solver() {
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> U(-1., 1.);
    std::normal_distribution<double> N(0., 1.);
    SolverStats st;
    double a[5][2], b[5][2];
    for (int trial = 0; trial < 2400; ++trial) {
        const int kind = trial % 4;  // 0: exact, 1: 0.3 px noise, 2: one gross outlier, 3: unrelated points
        const Scene s = make_motion(rng, false);
        for (int q = 0; q < 5; ++q) {
            const double X[3] = {10. * U(rng), 2. * U(rng), 22.5 + 17.5 * U(rng)};
            project(s, X, a[q], b[q]);
            if (kind >= 1)
                for (int c = 0; c < 2; ++c) b[q][c] += 0.3 / 718.856 * N(rng);
            if (kind == 3 || (kind == 2 && q == 4)) {
                b[q][0] = 0.8 * U(rng);
                b[q][1] = 0.25 * U(rng);
            }
        }
        check_sample(a, b, st, "random");
    }
    const int n_random = st.samples;
    CHECK(n_random >= 2000, "%d random samples", n_random);
    for (int trial = 0; trial < 40; ++trial) {  // five coplanar points (a fronto-parallel and a slanted plane)
        const Scene s = make_motion(rng, false);
        for (int q = 0; q < 5; ++q) {
            const double x = 10. * U(rng), y = 2. * U(rng);
            const double X[3] = {x, y, trial % 2 ? 20. + 0.3 * x - 0.2 * y : 20.};
            project(s, X, a[q], b[q]);
        }
        check_sample(a, b, st, "coplanar");
    }
    for (int trial = 0; trial < 40; ++trial) {  // pure rotation
        const Scene s = make_motion(rng, true);
        for (int q = 0; q < 5; ++q) {
            const double X[3] = {10. * U(rng), 2. * U(rng), 22.5 + 17.5 * U(rng)};
            project(s, X, a[q], b[q]);
        }
        check_sample(a, b, st, "pure rotation");
    }
    for (int trial = 0; trial < 40; ++trial) {  // two identical correspondences
        const Scene s = make_motion(rng, false);
        for (int q = 0; q < 5; ++q) {
            const double X[3] = {10. * U(rng), 2. * U(rng), 22.5 + 17.5 * U(rng)};
            project(s, X, a[q], b[q]);
        }
        a[3][0] = a[1][0];
        a[3][1] = a[1][1];
        b[3][0] = b[1][0];
        b[3][1] = b[1][1];
        check_sample(a, b, st, "two identical");
    }
    for (int trial = 0; trial < 10; ++trial) {  // five identical points (with and without flow; at the principal point)
        const double p[2] = {trial == 0 ? 0. : 0.5 * U(rng), trial == 0 ? 0. : 0.2 * U(rng)}, d = trial % 2 ? 0.01 : 0.;
        for (int q = 0; q < 5; ++q) {
            a[q][0] = p[0];
            a[q][1] = p[1];
            b[q][0] = p[0] + d;
            b[q][1] = p[1];
        }
        check_sample(a, b, st, "five identical");
    }
    std::printf("minimal solver: %d samples (%d random), %d models, %d samples without a model, %d with four or more\n", st.samples, n_random,
                st.models, st.zero, st.four_or_more);
    // the set proves nothing unless it holds both ends
    CHECK(st.zero >= 1, "no sample without a model");
    CHECK(st.four_or_more >= 1, "no sample with four or more models");
}

// ---- 2. the chunked pipeline
struct Matches {
    std::vector<kb::Vector2d> a, b;  // pixels
};
static const double kFocal = 718.856, kCx = 607.1928, kCy = 185.2157;
static Matches make_matches(uint64_t seed, int n, double outlier_share) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(-1., 1.);
    std::normal_distribution<double> N(0., 1.);
    const Scene s = make_motion(rng, false);
    Matches m;
    for (int i = 0; i < n; ++i) {
        const double X[3] = {10. * U(rng), 2. * U(rng), 22.5 + 17.5 * U(rng)};
        double a[2], b[2];
        project(s, X, a, b);
        kb::Vector2d pa(kFocal * a[0] + kCx, kFocal * a[1] + kCy), pb(kFocal * b[0] + kCx + 0.3 * N(rng), kFocal * b[1] + kCy + 0.3 * N(rng));
        if (0.5 * (U(rng) + 1.) < outlier_share) pb = kb::Vector2d(kCx + 600. * U(rng), kCy + 180. * U(rng));
        m.a.push_back(pa);
        m.b.push_back(pb);
    }
    return m;
}

// what limo_five_point does, on the host: the device kernels' statements in their order, the host statements as the library has them
static kb::five_point::Motion pipeline(const Matches& mt, double probability, double threshold_px, uint64_t seed, int max_samples, int chunk,
                                       std::vector<char>& mask) {
    kb::five_point::Motion m;
    const int n = (int)mt.a.size();
    mask.assign(n, 0);
    if (n < 5) return m;
    std::vector<double> pts(4 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        pts[4 * i] = fp5::normalise(mt.a[i][0], kCx, kFocal);
        pts[4 * i + 1] = fp5::normalise(mt.a[i][1], kCy, kFocal);
        pts[4 * i + 2] = fp5::normalise(mt.b[i][0], kCx, kFocal);
        pts[4 * i + 3] = fp5::normalise(mt.b[i][1], kCy, kFocal);
    }
    const double thr2 = (threshold_px / kFocal) * (threshold_px / kFocal);
    std::vector<int32_t> picks(5 * (size_t)max_samples);
    fp5::draw_picks(seed, n, max_samples, picks.data());
    fp5::Scan sc;
    fp5::scan_begin(sc, max_samples);
    double best_E[9] = {0};
    std::vector<double> models;
    std::vector<int32_t> n_models, counts;
    for (int start = 0; !sc.done;) {
        const int len = std::min(chunk, max_samples - start);
        models.assign(90 * (size_t)len, 0.);
        n_models.assign(len, 0);
        counts.assign(10 * (size_t)len, 0);
        for (int j = 0; j < len; ++j) {  // k_fp_models
            double ws[fp5::kWs], sa[10], sb[10];
            for (int q = 0; q < 5; ++q) {
                const double* p = pts.data() + 4 * (size_t)picks[5 * (size_t)(start + j) + q];
                sa[2 * q] = p[0];
                sa[2 * q + 1] = p[1];
                sb[2 * q] = p[2];
                sb[2 * q + 1] = p[3];
            }
            n_models[j] = fp5::essential_from_five(sa, sb, ws, models.data() + 90 * (size_t)j);
        }
        for (int j = 0; j < len; ++j)  // k_fp_score
            for (int k = 0; k < n_models[j]; ++k)
                for (int i = 0; i < n; ++i)
                    counts[10 * j + k] += fp5::sampson2(models.data() + 90 * (size_t)j + 9 * k, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], pts[4 * i + 3]) < thr2;
        const int bs = sc.best_sample, bm = sc.best_model;
        fp5::scan_chunk(sc, n, probability, max_samples, start, len, n_models.data(), counts.data());
        if (sc.best_sample != bs || sc.best_model != bm) std::memcpy(best_E, models.data() + 90 * (size_t)(sc.best_sample - start) + 9 * sc.best_model, sizeof(best_E));
        start += len;
    }
    m.samples = sc.samples;
    if (!sc.ok) return m;
    m.ok = true;
    m.inliers = sc.inliers;
    std::memcpy(m.E.data(), best_E, sizeof(best_E));
    double ws[24], cand[48];  // k_fp_pose
    fp5::pose_candidates(best_E, ws, cand);
    int front[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        const bool in = fp5::sampson2(best_E, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], pts[4 * i + 3]) < thr2;
        mask[i] = in;
        if (!in) continue;
        for (int c = 0; c < 4; ++c) front[c] += fp5::in_front(cand + 12 * c, cand + 12 * c + 9, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], pts[4 * i + 3]);
    }
    int best = -1;
    for (int c = 0; c < 4; ++c)
        if (front[c] > best) {
            best = front[c];
            std::memcpy(m.R.data(), cand + 12 * c, sizeof(double) * 9);
            std::memcpy(m.t, cand + 12 * c + 9, sizeof(double) * 3);
            m.in_front = front[c];
        }
    return m;
}

// five_point::estimateMotion keeps its mask to itself: the same statement (five_point.hpp:614) on its E
static std::vector<char> host_mask(const Matches& mt, const kb::five_point::Motion& m, double threshold_px) {
    const int n = (int)mt.a.size();
    std::vector<char> mask(n, 0);
    if (!m.ok) return mask;
    const double thr2 = (threshold_px / kFocal) * (threshold_px / kFocal);
    for (int i = 0; i < n; ++i) {
        const double a[2] = {(mt.a[i][0] - kCx) / kFocal, (mt.a[i][1] - kCy) / kFocal}, b[2] = {(mt.b[i][0] - kCx) / kFocal, (mt.b[i][1] - kCy) / kFocal};
        mask[i] = kb::five_point::sampson2(m.E, a, b) < thr2;
    }
    return mask;
}

static void test_pipeline() {
    int low = 0, mid = 0, at_cap = 0, cases = 0;
    const int ns[5] = {5, 6, 64, 65, 300};
    struct Cfg {
        double share;
        int max_samples;
    };
    const Cfg cfgs[4] = {{0.1, 1000}, {0.3, 1000}, {0.5, 1000}, {0.5, 50}};
    for (const Cfg& cfg : cfgs)
        for (int n : ns) {
            const uint64_t seed = 1000 + 17 * (uint64_t)n + (uint64_t)(cfg.share * 10);
            const Matches mt = make_matches(seed, n, cfg.share);
            const kb::five_point::Motion want = kb::five_point::estimateMotion(mt.a, mt.b, kFocal, kb::Vector2d(kCx, kCy), 0.999, 2.0, seed, cfg.max_samples);
            const std::vector<char> want_mask = host_mask(mt, want, 2.0);
            low += want.samples <= 64 && want.samples < cfg.max_samples;
            mid += want.samples > 64 && want.samples < cfg.max_samples;
            at_cap += want.samples == cfg.max_samples;
            std::printf("pipeline: n %3d outlier share %.1f cap %4d: ok %d samples %4d inliers %3d in front %3d\n", n, cfg.share, cfg.max_samples, (int)want.ok,
                        want.samples, want.inliers, want.in_front);
            const int chunks[4] = {1, 7, 64, cfg.max_samples};
            for (int chunk : chunks) {
                std::vector<char> mask;
                const kb::five_point::Motion got = pipeline(mt, 0.999, 2.0, seed, cfg.max_samples, chunk, mask);
                CHECK(got.ok == want.ok && got.inliers == want.inliers && got.in_front == want.in_front && got.samples == want.samples,
                      "n %d share %.1f cap %d chunk %d: ok %d/%d inliers %d/%d in_front %d/%d samples %d/%d", n, cfg.share, cfg.max_samples, chunk, (int)got.ok,
                      (int)want.ok, got.inliers, want.inliers, got.in_front, want.in_front, got.samples, want.samples);
                CHECK(same_bits(got.E.data(), want.E.data(), 9), "n %d share %.1f chunk %d: E differs", n, cfg.share, chunk);
                CHECK(same_bits(got.R.data(), want.R.data(), 9), "n %d share %.1f chunk %d: R differs", n, cfg.share, chunk);
                CHECK(same_bits(got.t, want.t, 3), "n %d share %.1f chunk %d: t differs", n, cfg.share, chunk);
                CHECK(mask == want_mask, "n %d share %.1f chunk %d: inlier mask differs", n, cfg.share, chunk);
                ++cases;
            }
        }
    {   // fewer than five matches: the initial Motion
        const Matches mt = make_matches(5, 4, 0.);
        std::vector<char> mask;
        const kb::five_point::Motion got = pipeline(mt, 0.999, 2.0, 1, 1000, 64, mask), want = kb::five_point::estimateMotion(mt.a, mt.b, kFocal, kb::Vector2d(kCx, kCy));
        CHECK(!got.ok && !want.ok && got.samples == 0 && same_bits(got.R.data(), want.R.data(), 9) && same_bits(got.t, want.t, 3), "n = 4");
    }
    std::printf("pipeline: %d cases; reference runs that stopped within 64 samples: %d, later but below the cap: %d, at the cap: %d\n", cases, low, mid, at_cap);
    CHECK(low >= 1, "no reference run stopped within 64 samples");
    CHECK(mid >= 1, "no reference run stopped between 64 samples and the cap");
    CHECK(at_cap >= 1, "no reference run reached the cap");
}

int main() {
    test_minimal_solver();
    test_pipeline();
    if (g_fail) {
        std::printf("%d of %d checks FAILED\n", g_fail, g_checks);
        return 1;
    }
    std::printf("all checks passed (%d)\n", g_checks);
    return 0;
}
