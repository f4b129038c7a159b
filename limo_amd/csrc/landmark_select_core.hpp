// landmark_select_core.hpp — landmark selection in front of a windowed solve, one statement for the host and for gfx950 lanes.
//
// Restates the selector the node wires (keyframe_bundle_adjustment/src/bundle_adjuster_keyframes.cpp:118 cheirality first;
// keyframe_bundle_adjustment_ros_tool/src/mono_lidar/mono_lidar.cpp:396-430 voxel sparsification + "depth assurance") as the host
// classes of this package state it - limo_amd/kba/landmark_selector.hpp:LandmarkRejectionSchemeCheirality::kept,
// landmark_selection_voxel.hpp:LandmarkSparsificationSchemeVoxel::categorized / LandmarkSelectionSchemeAddDepth::picked, wired by
// stream_driver.hpp:110-125 - on plain arrays, so that a lane of landmark_select.hip and the host give the same bytes.  Those
// classes, compiled with contraction off, stay the checker of this file (tests/cpp/landmark_select_ref.cpp).
// BIT-EXACT CONTRACT: floating-point contraction off on both sides (#pragma clang fp contract(off) + -ffp-contract=off in the
// build, as for five_point_core.hpp); every operation is one of + - * / sqrt floor fabs or a comparison, no sum is reassociated,
// and std::min / std::max are spelled as the comparisons they are (a NaN takes the branch it takes there).
//
// A pool arrives PACKED (landmark_select.hip:run, or select_pool_host below): keyframe and camera transforms formed once (T = [R row-major | t], the
// un-normalised polynomial rotation of convert(Pose)), the driven path in the newest keyframe's frame, the observations sorted by
// (landmark, time rank of the keyframe, camera) with a row-start index per landmark.  Landmarks are in ascending id, so "the
// smaller id" is "the smaller index" everywhere below.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "kba_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace kba {
namespace lsel {

constexpr int kMaxKf = 64, kMaxCam = 8;  // documented limits of limo_landmark_select
constexpr double kDblMax = 1.7976931348623157e308;
constexpr uint64_t kNoKey = ~uint64_t(0);  // sort key of a landmark outside the pipe / order key of a landmark that does not run
constexpr long kCellOff = 1l << 20;        // packed cell indices lie in (-2^20, 2^20)

enum Status : uint8_t { kRejected = 0, kCut = 1, kPipe = 2, kFar = 3 };  // after stage 1
enum Predicate { kHasDepth = 0, kIsGround = 1 };
enum KeyKind { kKeyMeasuredDepth = 0, kKeyRange = 1 };

struct Add {  // = limo_select_add
    int32_t frame_index, count, predicate, key;
};
struct Params {
    double voxel[3];
    double roi_far, roi_middle;
    uint32_t max_near, max_middle, max_far;
    int32_t n_add;
};
struct Pool {  // one packed pool (pointers of the host or of the device)
    int32_t n_kf, n_cam, n_lm, n_obs;
    int32_t newest;             // first keyframe with the largest stamp
    uint64_t seed;              // its stamp
    const double* T_kf;         // [n_kf*12]
    const double* T_cam;        // [n_cam*12]
    const double* path;         // [n_kf*3] keyframe positions in the newest keyframe's frame, keyframe order
    const int32_t* kf_by_time;  // [n_kf] keyframe index of time rank r
    const uint64_t* lm_id;      // [n_lm]
    const double* lm_pos;       // [n_lm*3]
    const uint8_t* lm_flags;    // [n_lm] bit 0 has_measured_depth, bit 1 is_ground_plane
    const int32_t* lm_obs;      // [n_lm+1] first observation of a landmark
    const int32_t* obs_rank;    // [n_obs] time rank of the keyframe
    const int32_t* obs_cam;
    const float *obs_u, *obs_v, *obs_d;
};

// ---- transforms (definitions.hpp:75-92)
KBA_HD void pose_T(const double* pose7, double* T) {  // convert(Pose): quat_R is NOT normalised
    quat_R(pose7, T);
    T[9] = pose7[4];
    T[10] = pose7[5];
    T[11] = pose7[6];
}
KBA_HD void apply(const double* T, const double* p, double* o) {  // EigenPose::operator*(Vector3d)
    o[0] = T[0] * p[0] + T[1] * p[1] + T[2] * p[2] + T[9];
    o[1] = T[3] * p[0] + T[4] * p[1] + T[5] * p[2] + T[10];
    o[2] = T[6] * p[0] + T[7] * p[1] + T[8] * p[2] + T[11];
}
KBA_HD void path_point(const double* cur, const double* Tk, double* o) {  // cur * Tk.inverse().translation()
    double it[3];
    for (int i = 0; i < 3; ++i) it[i] = -(Tk[i] * Tk[9] + Tk[3 + i] * Tk[10] + Tk[6 + i] * Tk[11]);
    apply(cur, it, o);
}
KBA_HD double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// landmark_helpers::distanceToPath
KBA_HD double dist_to_path(const double* p, const double* path, int n) {
    if (n == 0) return kDblMax;
    if (n == 1) return norm3(p[0] - path[0], p[1] - path[1], p[2] - path[2]);
    double best = kDblMax;
    for (int i = 0; i + 1 < n; ++i) {
        const double* a = path + 3 * i;
        const double* b = a + 3;
        const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
        const double l2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2];
        double t = l2 > 0. ? (ap[0] * ab[0] + ap[1] * ab[1] + ap[2] * ab[2]) / l2 : 0.;
        t = (0. < t) ? t : 0.;  // std::max(0., t)
        t = (t < 1.) ? t : 1.;  // std::min(1., .)
        const double d = norm3(p[0] - (a[0] + ab[0] * t), p[1] - (a[1] + ab[1] * t), p[2] - (a[2] + ab[2] * t));
        best = (d < best) ? d : best;
    }
    return best;
}

// the three cell indices of a pipe member; false when one lies outside (-2^20, 2^20) (the packed key does not hold it)
KBA_HD bool cell_of(const double* p, const double* voxel, double* c) {
    c[0] = floor(p[0] / voxel[0]);
    c[1] = floor(p[1] / voxel[1]);
    c[2] = floor(p[2] / voxel[2]);
    const double off = (double)kCellOff;
    return c[0] > -off && c[0] < off && c[1] > -off && c[1] < off && c[2] > -off && c[2] < off;
}
KBA_HD uint64_t cell_key(const double* c) {
    return ((uint64_t)((long)c[0] + kCellOff) << 42) | ((uint64_t)((long)c[1] + kCellOff) << 21) | (uint64_t)((long)c[2] + kCellOff);
}

// ---- order keys: the SMALLER (key, landmark index) wins
KBA_HD uint64_t bits_of(double x) {
    uint64_t b;
    memcpy(&b, &x, sizeof(b));
    return b;
}
KBA_HD uint64_t ord_ascending(double x) {  // orders like < on doubles (-0 = +0)
    if (x == 0.) x = 0.;
    const uint64_t b = bits_of(x);
    const uint64_t k = (b >> 63) ? ~b : (b | (uint64_t(1) << 63));
    return k == kNoKey ? kNoKey - 1 : k;
}
KBA_HD uint64_t ord_descending(double x) {
    const uint64_t k = ~ord_ascending(x);
    return k == kNoKey ? kNoKey - 1 : k;
}
KBA_HD uint64_t middle_rank(uint64_t id, uint64_t seed) {  // chooseMiddleLmIds
    uint64_t x = id * 0x9E3779B97F4A7C15ull + seed;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x = x ^ (x >> 31);
    return x == kNoKey ? kNoKey - 1 : x;  // (kNoKey is taken; a rank of 2^64 - 1 would have lost every comparison but one anyway)
}

// ---- stage 1, per landmark: cheirality, position in the newest keyframe's frame, plausibility cut, pipe / far, cell
struct Stage1 {
    uint8_t status;
    bool packed;   // (status == kPipe) the cell fits the packed key
    int32_t seen;  // keyframes that measured it
    double p[3], dist, cell[3];
};
KBA_HD void stage1(const Pool& P, const Params& prm, int i, Stage1* s) {
    const double* pos = P.lm_pos + 3 * (int64_t)i;
    bool bad = false;
    int seen = 0, last = -1;
    double pv[3] = {0., 0., 0.}, pc[3];
    for (int o = P.lm_obs[i]; o < P.lm_obs[i + 1]; ++o) {
        const int r = P.obs_rank[o];
        if (r != last) {
            apply(P.T_kf + 12 * P.kf_by_time[r], pos, pv);
            ++seen;
            last = r;
        }
        apply(P.T_cam + 12 * P.obs_cam[o], pv, pc);
        if (pc[2] < 0.) bad = true;
    }
    s->seen = seen;
    s->packed = true;
    s->dist = 0.;
    s->p[0] = s->p[1] = s->p[2] = 0.;
    s->cell[0] = s->cell[1] = s->cell[2] = 0.;
    if (bad) {
        s->status = kRejected;
        return;
    }
    apply(P.T_kf + 12 * P.newest, pos, s->p);
    if (!(s->p[2] >= -20. && s->p[2] <= 100.)) {
        s->status = kCut;
        return;
    }
    s->dist = dist_to_path(s->p, P.path, P.n_kf);
    if (s->dist < prm.roi_far) {
        s->status = kPipe;
        s->packed = cell_of(s->p, prm.voxel, s->cell);
    } else {
        s->status = kFar;
    }
}

// key of a must-have entry for landmark i in the keyframe of time rank `rank` (LandmarkSelectionSchemeAddDepth::picked):
// the largest key over the cameras that measured it there; false when the keyframe did not measure it
KBA_HD bool must_key(const Pool& P, int i, int rank, int key_kind, double* out) {
    bool found = false;
    double worst = -kDblMax;
    double local[3];
    float range = 0.f;
    for (int o = P.lm_obs[i]; o < P.lm_obs[i + 1]; ++o) {
        if (P.obs_rank[o] != rank) continue;
        if (!found && key_kind == kKeyRange) {
            apply(P.T_kf + 12 * P.kf_by_time[rank], P.lm_pos + 3 * (int64_t)i, local);
            range = (float)norm3(local[0], local[1], local[2]);
        }
        found = true;
        const double k = (double)(key_kind == kKeyRange ? range : P.obs_d[o]);
        worst = (worst < k) ? k : worst;  // std::max(worst, k)
    }
    *out = worst;
    return found;
}
KBA_HD bool predicate(uint8_t flags, int which) { return which == kIsGround ? (flags & 2) != 0 : (flags & 1) != 0; }

// ---- a voxel: members idx[c0 .. c1) in ascending landmark index, positions P3[3 * index]; the representative
// (landmark_selection_voxel.hpp:340-364: sequential centroid, nearest member, the 1e-9 relative tie rule as written)
KBA_HD uint32_t voxel_representative(const uint32_t* idx, int c0, int c1, const double* P3) {
    double sx = 0, sy = 0, sz = 0;
    for (int q = c0; q < c1; ++q) {
        const double* p = P3 + 3 * (int64_t)idx[q];
        sx += p[0];
        sy += p[1];
        sz += p[2];
    }
    const double n = (double)(c1 - c0);
    const double cx = sx / n, cy = sy / n, cz = sz / n;
    uint32_t best = idx[c0];
    double bd = kDblMax;
    for (int q = c0; q < c1; ++q) {
        const uint32_t i = idx[q];
        const double* p = P3 + 3 * (int64_t)i;
        const double d = norm3(p[0] - cx, p[1] - cy, p[2] - cz);
        const bool tie = fabs(d - bd) <= 1e-9 * (d + bd);
        if ((!tie && d < bd) || (tie && i < best)) {
            bd = d;
            best = i;
        }
    }
    return best;
}

// landmark_helpers::calcFlowSorted(.., use_mean = false) of one landmark: per camera the summed pixel displacement between
// consecutive keyframes (time order) that saw it, the largest over the cameras that saw it twice; false = no entry
KBA_HD bool flow_of(const Pool& P, int i, double* out) {
    double best = -1.;
    bool any = false;
    for (int c = 0; c < P.n_cam; ++c) {
        double sum = 0.;
        int cnt = 0;
        bool have = false;
        float lu = 0.f, lv = 0.f;
        for (int o = P.lm_obs[i]; o < P.lm_obs[i + 1]; ++o) {
            if (P.obs_cam[o] != c) continue;
            if (have) {
                const double du = double(lu) - double(P.obs_u[o]), dv = double(lv) - double(P.obs_v[o]);
                sum += sqrt(du * du + dv * dv);
                cnt += 1;
            }
            lu = P.obs_u[o];
            lv = P.obs_v[o];
            have = true;
        }
        if (cnt == 0) continue;
        any = true;
        best = (best < sum) ? sum : best;  // std::max(best, sum)
    }
    *out = best;
    return any;
}

// class (1 near, 2 middle) and order key of a voxel's representative; a near representative without a flow entry is not chosen
KBA_HD void classify_representative(const Pool& P, const Params& prm, int i, double dist, uint8_t* cls, uint64_t* ord) {
    if (dist < prm.roi_middle) {
        double f;
        const bool any = flow_of(P, i, &f);
        *cls = any ? 1 : 0;
        *ord = any ? ord_descending(f) : kNoKey;
    } else {
        *cls = 2;
        *ord = middle_rank(P.lm_id[i], P.seed);
    }
}
KBA_HD uint64_t far_ord(int n_kf, int seen) { return (uint64_t)(n_kf - seen); }  // the most keyframes first
KBA_HD uint32_t budget_of(const Params& prm, int cls) { return cls == 1 ? prm.max_near : cls == 2 ? prm.max_middle : prm.max_far; }

}  // namespace lsel
}  // namespace kba

// ---- host statements (plain host functions: the device pass only parses them)
#include <algorithm>
#include <array>
#include <utility>
#include <vector>

namespace kba {
namespace lsel {

// form the per-keyframe / per-camera parts of a packed pool: transforms, newest keyframe, path, time ranks
struct Frames {
    std::vector<double> T_kf, T_cam, path;
    std::vector<int32_t> kf_by_time, rank_of_kf;
    int32_t newest = 0;
    uint64_t seed = 0;
};
inline void make_frames(int n_kf, int n_cam, const double* kf_pose, const uint64_t* kf_stamp, const double* cam10, Frames* F) {
    F->T_kf.resize(12 * (size_t)n_kf);
    F->T_cam.resize(12 * (size_t)n_cam);
    F->path.resize(3 * (size_t)n_kf);
    F->kf_by_time.resize(n_kf);
    F->rank_of_kf.resize(n_kf);
    for (int k = 0; k < n_kf; ++k) pose_T(kf_pose + 7 * k, F->T_kf.data() + 12 * k);
    for (int c = 0; c < n_cam; ++c) pose_T(cam10 + 10 * c + 3, F->T_cam.data() + 12 * c);
    F->newest = 0;
    for (int k = 1; k < n_kf; ++k)
        if (kf_stamp[F->newest] < kf_stamp[k]) F->newest = k;  // std::max_element: the first largest
    F->seed = n_kf ? kf_stamp[F->newest] : 0;
    for (int k = 0; k < n_kf; ++k) {
        F->kf_by_time[k] = k;
        path_point(F->T_kf.data() + 12 * F->newest, F->T_kf.data() + 12 * k, F->path.data() + 3 * k);
    }
    std::stable_sort(F->kf_by_time.begin(), F->kf_by_time.end(), [&](int a, int b) { return kf_stamp[a] < kf_stamp[b]; });
    for (int r = 0; r < n_kf; ++r) F->rank_of_kf[F->kf_by_time[r]] = r;
}

// observations of one pool into (landmark, time rank, camera) order: rows start[n_lm + 1], order[n_obs] (indices into the caller's
// arrays).  A counting sort by landmark, then an insertion sort inside each landmark's few rows (linear on input that is already in
// order).  false = a (kf, lm, cam) twice.
inline bool order_observations(int n_lm, int n_obs, const int32_t* obs_kf, const int32_t* obs_lm, const int32_t* obs_cam, const int32_t* rank_of_kf,
                               int32_t* start, std::vector<int32_t>& order, int* dup_at) {
    std::fill(start, start + n_lm + 1, 0);
    for (int o = 0; o < n_obs; ++o) ++start[obs_lm[o] + 1];
    for (int i = 0; i < n_lm; ++i) start[i + 1] += start[i];
    std::vector<int32_t> fill(start, start + n_lm);
    order.resize(n_obs);
    for (int o = 0; o < n_obs; ++o) order[fill[obs_lm[o]]++] = o;
    auto key = [&](int32_t o) { return rank_of_kf[obs_kf[o]] * kMaxCam + obs_cam[o]; };
    for (int i = 0; i < n_lm; ++i) {
        for (int a = start[i] + 1; a < start[i + 1]; ++a) {
            const int32_t o = order[a];
            const int ko = key(o);
            int b = a;
            for (; b > start[i] && key(order[b - 1]) > ko; --b) order[b] = order[b - 1];
            order[b] = o;
        }
        for (int a = start[i] + 1; a < start[i + 1]; ++a)
            if (key(order[a]) == key(order[a - 1])) {
                *dup_at = order[a];
                return false;
            }
    }
    return true;
}

// the `budget` smallest (ord, index) of the landmarks of a class: out[index] |= bit
inline void take_smallest(std::vector<std::pair<uint64_t, int>>& keyed, int64_t budget, uint8_t bits, uint8_t* out) {
    std::sort(keyed.begin(), keyed.end());
    for (int64_t q = 0; q < budget && q < (int64_t)keyed.size(); ++q) out[keyed[q].second] |= bits;
}

// The whole selection of one packed pool, serially: what the kernels of landmark_select.hip compute, and what finishes a pool
// whose cell indices leave (-2^20, 2^20) (there the triples are compared, landmark_selection_voxel.hpp:325-337).
// out[n_lm]: low two bits category (1 near, 2 middle, 3 far), | 4 must-have, 8 = rejected by cheirality.
inline void select_host(const Pool& P, const Params& prm, const Add* add, uint8_t* out) {
    const int n = P.n_lm;
    std::fill(out, out + n, uint8_t(0));
    if (n == 0 || P.n_kf == 0) return;
    std::vector<Stage1> s(n);
    std::vector<double> p3(3 * (size_t)n);
    bool packed = true;
    for (int i = 0; i < n; ++i) {
        stage1(P, prm, i, &s[i]);
        for (int a = 0; a < 3; ++a) p3[3 * (size_t)i + a] = s[i].p[a];
        if (s[i].status == kPipe && !s[i].packed) packed = false;
        if (s[i].status == kRejected) out[i] = 8;
    }
    // voxels of the pipe: members by (cell, index)
    std::vector<uint32_t> idx;
    std::vector<int> seg;  // segment starts, closed by idx.size()
    if (packed) {
        std::vector<std::pair<uint64_t, uint32_t>> cells;
        for (int i = 0; i < n; ++i)
            if (s[i].status == kPipe) cells.push_back({cell_key(s[i].cell), (uint32_t)i});
        std::sort(cells.begin(), cells.end());
        for (size_t q = 0; q < cells.size(); ++q) {
            if (q == 0 || cells[q].first != cells[q - 1].first) seg.push_back((int)q);
            idx.push_back(cells[q].second);
        }
    } else {
        std::vector<std::pair<std::array<long, 3>, uint32_t>> wide;
        for (int i = 0; i < n; ++i)
            if (s[i].status == kPipe) wide.push_back({{{(long)s[i].cell[0], (long)s[i].cell[1], (long)s[i].cell[2]}}, (uint32_t)i});
        std::sort(wide.begin(), wide.end());
        for (size_t q = 0; q < wide.size(); ++q) {
            if (q == 0 || wide[q].first != wide[q - 1].first) seg.push_back((int)q);
            idx.push_back(wide[q].second);
        }
    }
    seg.push_back((int)idx.size());
    std::vector<std::pair<uint64_t, int>> keyed[4];
    for (size_t v = 0; v + 1 < seg.size(); ++v) {
        const int rep = (int)voxel_representative(idx.data(), seg[v], seg[v + 1], p3.data());
        uint8_t cls;
        uint64_t ord;
        classify_representative(P, prm, rep, s[rep].dist, &cls, &ord);
        if (cls) keyed[cls].push_back({ord, rep});
    }
    for (int i = 0; i < n; ++i)
        if (s[i].status == kFar) keyed[3].push_back({far_ord(P.n_kf, s[i].seen), i});
    for (int c = 1; c <= 3; ++c) take_smallest(keyed[c], (int64_t)budget_of(prm, c), (uint8_t)c, out);
    for (int e = 0; e < prm.n_add; ++e) {
        const Add& a = add[e];
        if (a.frame_index < 0 || a.frame_index > P.n_kf - 1) continue;
        std::vector<std::pair<uint64_t, int>> cand;
        for (int i = 0; i < n; ++i) {
            double k;
            if (s[i].status == kRejected || !predicate(P.lm_flags[i], a.predicate) || !must_key(P, i, a.frame_index, a.key, &k)) continue;
            cand.push_back({ord_ascending(k), i});
        }
        take_smallest(cand, (int64_t)a.count, 4, out);
    }
}

}  // namespace lsel
}  // namespace kba

namespace kba {
namespace lsel {

// A caller's pool (the arrays of limo_select_pool, already validated) packed on the host and selected with select_host: the serial
// form of limo_landmark_select (tests/cpp/test_landmark_select_core.cpp holds it against the host classes).  false = a duplicate
// (kf, lm, cam) observation.
inline bool select_pool_host(int n_kf, int n_cam, int n_lm, int n_obs, const double* kf_pose, const uint64_t* kf_stamp, const double* cam10,
                             const uint64_t* lm_id, const double* lm_pos, const uint8_t* lm_has_depth, const uint8_t* lm_is_ground,
                             const int32_t* obs_kf, const int32_t* obs_lm, const int32_t* obs_cam, const float* obs_u, const float* obs_v,
                             const float* obs_d, const Params& prm, const Add* add, uint8_t* out) {
    std::fill(out, out + n_lm, uint8_t(0));
    if (n_lm == 0 || n_kf == 0) return true;
    Frames F;
    make_frames(n_kf, n_cam, kf_pose, kf_stamp, cam10, &F);
    std::vector<int32_t> start((size_t)n_lm + 1), order, rank(n_obs), cm(n_obs);
    int dup = 0;
    if (!order_observations(n_lm, n_obs, obs_kf, obs_lm, obs_cam, F.rank_of_kf.data(), start.data(), order, &dup)) return false;
    std::vector<float> u(n_obs), v(n_obs), d(n_obs);
    std::vector<uint8_t> flags(n_lm);
    for (int a = 0; a < n_obs; ++a) {
        const int32_t o = order[a];
        rank[a] = F.rank_of_kf[obs_kf[o]], cm[a] = obs_cam[o], u[a] = obs_u[o], v[a] = obs_v[o], d[a] = obs_d[o];
    }
    for (int i = 0; i < n_lm; ++i) flags[i] = (lm_has_depth[i] ? 1 : 0) | (lm_is_ground[i] ? 2 : 0);
    Pool P;
    P.n_kf = n_kf, P.n_cam = n_cam, P.n_lm = n_lm, P.n_obs = n_obs, P.newest = F.newest, P.seed = F.seed;
    P.T_kf = F.T_kf.data(), P.T_cam = F.T_cam.data(), P.path = F.path.data(), P.kf_by_time = F.kf_by_time.data();
    P.lm_id = lm_id, P.lm_pos = lm_pos, P.lm_flags = flags.data(), P.lm_obs = start.data();
    P.obs_rank = rank.data(), P.obs_cam = cm.data(), P.obs_u = u.data(), P.obs_v = v.data(), P.obs_d = d.data();
    select_host(P, prm, add, out);
    return true;
}

}  // namespace lsel
}  // namespace kba
