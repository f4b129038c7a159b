// test_landmark_select_core.cpp — limo_amd/csrc/landmark_select_core.hpp run serially on the host (lsel::select_pool_host: pack +
// select_host, the statement the kernels of landmark_select.hip share) against the host classes (landmark_select_ref.cpp: Keyframe /
// Landmark objects and LandmarkSelector as StreamDriver wires it), byte for byte, on random pools of its own.  A stand-alone program:
// built plain and with -fsanitize=address,undefined by tests/landmark_select_common.py.
#include <cmath>
#include <cstdio>
#include <limits>

#include "landmark_select_ref.cpp"
#include "../../limo_amd/csrc/landmark_select_core.hpp"

namespace {

struct Rng {
    uint64_t s;
    double uni() {  // [0, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / 9007199254740992.0;
    }
    double in(double a, double b) { return a + (b - a) * uni(); }
    int below(int n) { return (int)(uni() * n); }
};

struct Scene {
    int n_kf, n_cam, n_lm;
    std::vector<double> kf_pose, cam, lm_pos;
    std::vector<uint64_t> kf_stamp, lm_id;
    std::vector<uint8_t> has_depth, is_ground;
    std::vector<int32_t> obs_kf, obs_lm, obs_cam;
    std::vector<float> u, v, d;
    limo_select_pool pool() const {
        limo_select_pool w;
        w.n_kf = n_kf, w.n_cam = n_cam, w.n_lm = n_lm, w.n_obs = (int)obs_kf.size();
        w.kf_pose = kf_pose.data(), w.kf_stamp = kf_stamp.data(), w.cam = cam.data();
        w.lm_id = lm_id.data(), w.lm_pos = lm_pos.data(), w.lm_has_depth = has_depth.data(), w.lm_is_ground = is_ground.data();
        w.obs_kf = obs_kf.data(), w.obs_lm = obs_lm.data(), w.obs_cam = obs_cam.data();
        w.obs_u = u.data(), w.obs_v = v.data(), w.obs_d = d.data();
        return w;
    }
};

// a vehicle driving along +z with a little yaw; landmarks around the path, some doubled (shared voxels), some behind old keyframes
Scene make_scene(uint64_t seed, int n_kf, int n_cam, int n_lm, bool stamps_descending) {
    Rng r{seed * 2654435761ull + 12345};
    Scene S;
    S.n_kf = n_kf, S.n_cam = n_cam, S.n_lm = n_lm;
    double zpos = 0.;
    for (int k = 0; k < n_kf; ++k) {
        const double yaw = 0.02 * k + r.in(-0.01, 0.01), c = std::cos(yaw / 2), s = std::sin(yaw / 2);
        const double q[4] = {c * r.in(0.999, 1.001), 0., s, 0.};  // (not exactly unit: the rotation is the polynomial one)
        double R[9];
        kba::quat_R(q, R);
        const double C[3] = {r.in(-0.3, 0.3), 0., zpos};
        zpos += r.in(0.5, 2.0);
        S.kf_pose.insert(S.kf_pose.end(), {q[0], q[1], q[2], q[3], -(R[0] * C[0] + R[1] * C[1] + R[2] * C[2]), -(R[3] * C[0] + R[4] * C[1] + R[5] * C[2]),
                                           -(R[6] * C[0] + R[7] * C[1] + R[8] * C[2])});
        S.kf_stamp.push_back(stamps_descending ? 1000000000ull * (uint64_t)(n_kf - k) : 1000000000ull + 100000000ull * (uint64_t)k);
    }
    for (int c = 0; c < n_cam; ++c) S.cam.insert(S.cam.end(), {718.856, 607.19, 185.21, 1., 0., 0., 0., -0.54 * c, 0., 0.});
    uint64_t id = 10;
    for (int i = 0; i < n_lm; ++i) {
        id += 1 + (uint64_t)r.below(3);
        S.lm_id.push_back(id);
        double p[3] = {r.in(-60., 60.), r.in(-2., 3.), zpos + r.in(-25., 130.)};
        if (i > 0 && r.uni() < 0.3)  // next to the landmark before: the same voxel more often than not
            for (int a = 0; a < 3; ++a) p[a] = S.lm_pos[3 * (i - 1) + a] + r.in(-0.2, 0.2);
        if (r.uni() < 0.01) p[r.below(3)] = r.uni() < 0.5 ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
        S.lm_pos.insert(S.lm_pos.end(), p, p + 3);
        S.has_depth.push_back(r.uni() < 0.4);
        S.is_ground.push_back(r.uni() < 0.2);
        const int k0 = r.below(n_kf), k1 = k0 + r.below(n_kf - k0 + 1);  // measured in keyframes [k0, k1): possibly none
        for (int k = k0; k < k1; ++k)
            for (int c = 0; c < n_cam; ++c) {
                if (c > 0 && r.uni() < 0.3) continue;
                double T[12], y[3];
                kba::lsel::pose_T(S.kf_pose.data() + 7 * k, T);
                kba::lsel::apply(T, p, y);
                const double z = std::fabs(y[2]) > 0.1 ? y[2] : 0.1;
                S.obs_kf.push_back(k), S.obs_lm.push_back(i), S.obs_cam.push_back(c);
                S.u.push_back((float)(718.856 * (y[0] - 0.54 * c) / z + 607.19 + r.in(-0.5, 0.5)));
                S.v.push_back((float)(718.856 * y[1] / z + 185.21 + r.in(-0.5, 0.5)));
                S.d.push_back(S.has_depth.back() && r.uni() < 0.7 ? (float)y[2] : -1.f);
            }
    }
    // any order: shuffle the observations
    for (int a = (int)S.obs_kf.size() - 1; a > 0; --a) {
        const int b = r.below(a + 1);
        std::swap(S.obs_kf[a], S.obs_kf[b]), std::swap(S.obs_lm[a], S.obs_lm[b]), std::swap(S.obs_cam[a], S.obs_cam[b]);
        std::swap(S.u[a], S.u[b]), std::swap(S.v[a], S.v[b]), std::swap(S.d[a], S.d[b]);
    }
    return S;
}

int failures = 0;

void check(const char* what, const Scene& S, const limo_select_params& q, int* histogram) {
    const limo_select_pool w = S.pool();
    std::vector<uint8_t> want(S.n_lm + 1), got(S.n_lm + 1);
    const int rc = landmark_select_ref(&w, &q, want.data(), nullptr, 0);
    kba::lsel::Params prm;
    for (int a = 0; a < 3; ++a) prm.voxel[a] = q.voxel_size_xyz[a];
    prm.roi_far = q.roi_far, prm.roi_middle = q.roi_middle, prm.max_near = q.max_near, prm.max_middle = q.max_middle, prm.max_far = q.max_far, prm.n_add = q.n_add;
    std::vector<kba::lsel::Add> add;
    for (int e = 0; e < q.n_add; ++e) add.push_back({q.add[e].frame_index, q.add[e].count, q.add[e].predicate, q.add[e].key});
    const bool ok = kba::lsel::select_pool_host(w.n_kf, w.n_cam, w.n_lm, w.n_obs, w.kf_pose, w.kf_stamp, w.cam, w.lm_id, w.lm_pos, w.lm_has_depth, w.lm_is_ground, w.obs_kf,
                                                w.obs_lm, w.obs_cam, w.obs_u, w.obs_v, w.obs_d, prm, add.data(), got.data());
    int diff = 0;
    for (int i = 0; i < S.n_lm; ++i) {
        diff += want[i] != got[i];
        ++histogram[want[i] & 15];
    }
    if (rc != 0 || !ok || diff) {
        ++failures;
        std::printf("FAIL %s: checker rc %d, pack ok %d, %d of %d bytes differ\n", what, rc, (int)ok, diff, S.n_lm);
    }
}

}  // namespace

int main() {
    int histogram[16] = {0};
    limo_select_add adds[6] = {{0, 5, LIMO_SELECT_HAS_DEPTH, LIMO_SELECT_KEY_MEASURED_DEPTH}, {0, 8, LIMO_SELECT_IS_GROUND, LIMO_SELECT_KEY_RANGE},
                               {1, 8, LIMO_SELECT_IS_GROUND, LIMO_SELECT_KEY_RANGE},          {2, 1000, LIMO_SELECT_IS_GROUND, LIMO_SELECT_KEY_RANGE},
                               {40, 8, LIMO_SELECT_IS_GROUND, LIMO_SELECT_KEY_RANGE},         {-1, 8, LIMO_SELECT_HAS_DEPTH, LIMO_SELECT_KEY_RANGE}};
    int cases = 0;
    for (int n_lm : {0, 1, 2, 7, 63, 64, 65, 300, 900})
        for (int n_kf : {0, 1, 2, 3, 12})
            for (int n_cam : {1, 2})
                for (uint64_t seed = 1; seed <= 2; ++seed) {
                    const Scene S = make_scene(seed * 1000 + n_lm * 7 + n_kf * 3 + n_cam, n_kf, n_cam, n_lm, seed == 2);
                    for (int variant = 0; variant < 4; ++variant) {
                        limo_select_params q;
                        q.voxel_size_xyz[0] = 0.5, q.voxel_size_xyz[1] = 0.5, q.voxel_size_xyz[2] = 0.3;
                        q.roi_far = 40., q.roi_middle = 15.;
                        q.max_near = 200, q.max_middle = 200, q.max_far = 100;
                        q.n_add = 6, q.add = adds, q.sort_capacity = 0;
                        if (variant == 1) q.max_near = (uint32_t)(n_lm / 20), q.max_middle = (uint32_t)(n_lm / 20), q.max_far = (uint32_t)(n_lm / 30);  // budgets bind (or are 0)
                        if (variant == 2) q.voxel_size_xyz[0] = q.voxel_size_xyz[1] = q.voxel_size_xyz[2] = 1e-5;  // cells beyond +-2^20: the triples
                        if (variant == 3) q.voxel_size_xyz[0] = q.voxel_size_xyz[1] = q.voxel_size_xyz[2] = 500., q.n_add = 0;  // one voxel
                        char what[128];
                        std::snprintf(what, sizeof(what), "n_lm %d n_kf %d n_cam %d seed %d variant %d", n_lm, n_kf, n_cam, (int)seed, variant);
                        check(what, S, q, histogram);
                        ++cases;
                    }
                }
    std::printf("%d pools; checker's bytes: none %d near %d middle %d far %d must-have only %d near+must %d middle+must %d far+must %d rejected %d\n", cases, histogram[0],
                histogram[1], histogram[2], histogram[3], histogram[4], histogram[5], histogram[6], histogram[7], histogram[8]);
    // a test that compares empty selections shows nothing
    for (int b : {1, 2, 3, 4, 8})
        if (histogram[b] == 0) {
            std::printf("FAIL: no pool gave a byte of value %d\n", b);
            ++failures;
        }
    std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
