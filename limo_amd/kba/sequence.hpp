// sequence.hpp — one sequence's frame pipeline: what a frame does, in which order and under which conditions, stated once for the two
// drivers.  The call order is the reference node's,
//   keyframe_bundle_adjustment_ros_tool/src/mono_lidar/mono_lidar.cpp:88-373 (MonoLidar::callbackSubscriber)
// with the depth assignment of the (separate) tracklets_depth node in front of it:
//   LiDAR sweep + tracked features of the frame
//     -> depth of every track's newest point (the sweep), of its older points (the depth history)
//     -> motion prior                   external (the node: tf), else the five-point direction scaled by the last keyframes'
//                                       speed (:157-186, five_point.hpp; StreamParams::motion_prior) or - the default here -
//                                       constant velocity from the last two poses
//     -> Keyframe(prior) + adjustPoseOnly            (:192-211)
//     -> KeyframeSelector::select                    (:218-222)
//     -> push                                        (:231-233)
//     -> deactivateKeyframes + updateLabels + solve  (:245-263, every time_between_keyframes)
//     -> pose of the frame in KITTI form             (:281-294: camera_0 <- camera_t, 12 numbers per row)
// The very first frame is a Pose-fixed keyframe at the identity (:305-326).
// stream_detail::Sequence holds a sequence's state and the HOST phases of a frame; between two phases stands a device call that the
// driver makes: StreamDriver (stream_driver.hpp) one call per sequence on the adjuster's own context, LockstepDriver
// (lockstep_driver.hpp) one batched call for all its sequences.  Everything numerical happens behind the C-ABI.
#pragma once
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ostream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/limo_hip.h"
#include "bundle_adjuster_keyframes.hpp"
#include "five_point.hpp"
#include "keyframe_selector.hpp"
#include "kitti_io.hpp"
#include "landmark_selection_voxel.hpp"

namespace keyframe_bundle_adjustment {

struct StreamParams {
    // optimisation window (MonoLidar.rosif / keyframe_ba_monolid.launch)
    int max_size_optimization_window = 5;
    int min_number_connecting_landmarks = 3;
    double time_between_keyframes_sec = 0.09;   // solve at most this often (:245), also the time sparsification scheme
    double critical_rotation_difference = 0.1;  // KeyframeSelectionSchemePose
    double min_median_flow = 3.;                // KeyframeRejectionSchemeFlow
    double shrubbery_weight = 0.9;
    double height_over_ground = 0.31;           // Plane::distance of new keyframes (:191)
    double solver_time_sec = 20.;               // wall-clock cap of a solve; <= 0: none (deterministic)
    double prior_speed = 11.;                   // m/s along the vehicle's x axis while no motion has been estimated yet (the
                                                // node scales its five-point direction by interface_.prior_speed, :160-165)
    // outlier rejection of solve() and adjustPoseOnly() (keyframe_ba_monolid.launch:41-46; the node writes them into
    // BundleAdjusterKeyframes::outlier_rejection_options_, and so does the sequence): the defaults are OutlierRejectionOptions' own.
    // What the reference's tune_parameters_kitti.py sweeps.
    double robust_loss_depth_thres = 0.16;        // Cauchy scale of the depth blocks
    double robust_loss_reprojection_thres = 1.6;  // ... of the reprojection blocks
    double outlier_rejection_quantile = 0.95;     // both quantiles of the trimming rounds
    int outlier_rejection_num_iterations = 1;     // trimming rounds (part of the schedule)
    // Motion prior of a frame that comes without an external one (mono_lidar.cpp:157-186): the node takes the direction from
    // the five-point algorithm on the matches between the last keyframe and the frame and the length from the speed of the last
    // two keyframes (five_point.hpp restates it); constant velocity from the last two frame poses is this driver's default (no
    // RANSAC in the frame loop; adjustPoseOnly refines either against the fixed landmarks).
    enum class MotionPrior { ConstantVelocity, FivePoint };
    MotionPrior motion_prior = MotionPrior::ConstantVelocity;
    // Where the five-point estimate of MotionPrior::FivePoint is computed: limo_five_point (the device: every minimal sample of a round
    // at once) where the library behind the C-ABI has it, else - and always with `false` - five_point::estimateMotion on the host.
    // The two give the same Motion bit for bit, hence the same pose rows.  The default follows the measurement of BASELINE.md §4.16
    // (at a third of the matches wrong the device call is 3 - 5 x the host's).
    bool five_point_on_device = false;
    // Where solve() selects its landmarks: limo_landmark_select (the device; BundleAdjusterKeyframes::setDeviceSelection, with the values
    // below) where the library behind the C-ABI has it, else - and always with `false` - the host selector.  The two give the same
    // selection, hence the same pose rows.  The default follows the measurement of BASELINE.md §4.17.
    bool landmark_selection_on_device = false;
    // Marginal covariance of every refined frame pose (not in the reference; include/limo_hip.h, "Pose covariance"): the frame's
    // adjustPoseOnly ends with the library's covariance pass and the sequence keeps its 6 x 6 block and status per frame
    // (Sequence::covariances, writeCovariances).  No pose changes with it.
    bool pose_covariance = false;
    // landmark selection (keyframe_ba_monolid.launch:36-38; wiring of MonoLidar::reconfigureRequest, mono_lidar.cpp:396-430)
    unsigned max_number_landmarks_near_bin = 200, max_number_landmarks_middle_bin = 200, max_number_landmarks_far_bin = 100;
    double roi_middle = 15., roi_far = 40.;                            // :405-408
    std::array<double, 3> voxel_size_xyz{{0.5, 0.5, 0.3}};             // :404
    int add_ground_landmarks_per_keyframe = 50;                        // :421-423: for EVERY index of the window the 50
                                                                       // nearest ground-plane landmarks are kept
    int add_depth_landmarks_newest = 0;                                // the node has this rule commented out (:412-416)
    // depth assignment
    bool assign_depth = true;
    // How the depth assignment of a frame announced with announceNextFrame runs ahead of the frame before it (the reference's depth
    // estimator is a process of its own beside the BA node, kitti_standalone.launch:14-23, :55: it works on frame t+1 while the
    // bundle adjuster works on frame t):
    //   Thread  a thread of this driver - the "depth node" - does all of it (limo_depth_estimate on the driver's own context, the
    //           per-track depth history, the depth of every point of the tracker's message as one array the calling thread copies
    //           into the message when it takes the frame) while the calling thread runs frame t
    //   Stream  the calling thread starts it (limo_depth_estimate_begin: copies and kernels on the driver's own stream) and collects
    //           it at the start of the next process() call (limo_depth_estimate_end): no second thread, only the GPU time is hidden
    //   None    announceNextFrame is ignored
    // The results are the same bits in all three.
    enum class DepthAhead { None, Stream, Thread };
    DepthAhead depth_ahead = DepthAhead::Thread;
    int image_width = 1241, image_height = 376;
    std::vector<int> ground_labels{6, 7, 8, 9, 10};  // cityscapes labels treated as ground (labels_["ground"])
};

// Counts and host seconds of one sequence (StreamDriver::Stats).  The phases of stream_detail::Sequence time their own statements into
// the sec_ figures; what a driver's device call takes, the driver adds: StreamDriver does, so its figures cover whole stages;
// LockstepDriver times its batched calls per stage (LockstepDriver::Stage), so there these are the host halves alone.
struct StreamStats {
    int frames = 0, keyframes = 0, solves = 0, solves_on_non_keyframes = 0, features = 0, features_with_depth = 0, depth_prefetched = 0;
    double sec_depth = 0., sec_pose_only = 0., sec_push = 0., sec_solve = 0., sec_total = 0.;
    // host-side bookkeeping of a frame: the Keyframe object of the frame (measurement maps of its tracks), keyframe
    // selection, window cut + labels; and of sec_pose_only / sec_solve the share spent inside the C-ABI calls
    double sec_keyframe = 0., sec_select = 0., sec_window = 0., sec_abi_pose_only = 0., sec_abi_solve = 0., sec_depth_history = 0.;
    double sec_depth_thread = 0.;  // time the depth thread worked (beside the calling thread: not part of sec_total)
    int five_point_calls = 0, five_point_device_calls = 0;  // estimates of the five-point prior, and how many of them limo_five_point made
    double sec_five_point = 0.;
};

namespace stream_detail {

// adds the time of its scope to one of the figures above
class Timed {
public:
    explicit Timed(double& sec) : sec_(sec), t0_(std::chrono::steady_clock::now()) {}
    ~Timed() { sec_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count(); }
    Timed(const Timed&) = delete;
    Timed& operator=(const Timed&) = delete;

private:
    double& sec_;
    std::chrono::steady_clock::time_point t0_;
};
template <class F>
auto timed(double& sec, F&& fn) -> decltype(fn()) {  // ... the time of fn()
    Timed t(sec);
    return fn();
}

// the node's wiring of keyframe selection and landmark selection (mono_lidar.cpp:396-430) for one sequence's adjuster
inline void configureSequence(const StreamParams& p, BundleAdjusterKeyframes& ba, KeyframeSelector& selector) {
    ba.set_solver_time(p.solver_time_sec);
    ba.setPoseCovariance(p.pose_covariance);
    ba.outlier_rejection_options_.depth_thres = p.robust_loss_depth_thres;
    ba.outlier_rejection_options_.reprojection_thres = p.robust_loss_reprojection_thres;
    ba.outlier_rejection_options_.depth_quantile = p.outlier_rejection_quantile;
    ba.outlier_rejection_options_.reprojection_quantile = p.outlier_rejection_quantile;
    ba.outlier_rejection_options_.num_iterations = p.outlier_rejection_num_iterations;
    selector.addScheme(KeyframeRejectionSchemeFlow::createConst(p.min_median_flow));
    selector.addScheme(KeyframeSelectionSchemePose::createConst(p.critical_rotation_difference));
    selector.addScheme(KeyframeSparsificationSchemeTime::createConst(p.time_between_keyframes_sec * 1e9));
    LandmarkSparsificationSchemeVoxel::Parameters vp;
    vp.max_num_landmarks_near = p.max_number_landmarks_near_bin;
    vp.max_num_landmarks_middle = p.max_number_landmarks_middle_bin;
    vp.max_num_landmarks_far = p.max_number_landmarks_far_bin;
    vp.voxel_size_xyz = p.voxel_size_xyz;
    vp.roi_far_xyz = {{p.roi_far, p.roi_far, p.roi_far}};
    vp.roi_middle_xyz = {{p.roi_middle, p.roi_middle, p.roi_middle}};
    ba.landmark_selector_->addScheme(LandmarkSparsificationSchemeVoxel::createConst(vp));
    LandmarkSelectionSchemeAddDepth::Parameters ap;  // "depth assurance" (:409-426)
    if (p.add_depth_landmarks_newest > 0)
        ap.params_per_keyframe.push_back(std::make_tuple(0, p.add_depth_landmarks_newest, [](const Landmark::ConstPtr& lm) { return lm->has_measured_depth; },
                                                         [](const Measurement& m, const Vector3d&) { return m.d; }));
    for (int i = 0; i < p.max_size_optimization_window && p.add_ground_landmarks_per_keyframe > 0; ++i)
        ap.params_per_keyframe.push_back(std::make_tuple(i, p.add_ground_landmarks_per_keyframe, [](const Landmark::ConstPtr& lm) { return lm->is_ground_plane; },
                                                         [](const Measurement&, const Vector3d& local) { return (float)local.norm(); }));
    ba.landmark_selector_->addScheme(LandmarkSelectionSchemeAddDepth::createConst(ap));
    if (p.landmark_selection_on_device) {  // the same wiring as limo_select_params (the host schemes above stay: they take over when the call is refused)
        limo_select_params sp{};
        for (int i = 0; i < 3; ++i) sp.voxel_size_xyz[i] = p.voxel_size_xyz[i];
        sp.roi_far = p.roi_far, sp.roi_middle = p.roi_middle;
        sp.max_near = p.max_number_landmarks_near_bin, sp.max_middle = p.max_number_landmarks_middle_bin, sp.max_far = p.max_number_landmarks_far_bin;
        std::vector<limo_select_add> add;
        if (p.add_depth_landmarks_newest > 0) add.push_back({0, p.add_depth_landmarks_newest, LIMO_SELECT_HAS_DEPTH, LIMO_SELECT_KEY_MEASURED_DEPTH});
        for (int i = 0; i < p.max_size_optimization_window && p.add_ground_landmarks_per_keyframe > 0; ++i)
            add.push_back({i, p.add_ground_landmarks_per_keyframe, LIMO_SELECT_IS_GROUND, LIMO_SELECT_KEY_RANGE});
        sp.n_add = (int32_t)add.size(), sp.add = add.data();
        ba.setDeviceSelection(&sp);
    }
}

// pixel coordinates and ground flags of the newest point of every track, as limo_depth_estimate wants them
inline void stageFeatures(const StreamParams& p, const Tracklets& ts, std::vector<float>& uv, std::vector<uint8_t>& ground) {
    const size_t n = ts.tracks.size();
    uv.resize(2 * n);
    ground.resize(n);
    for (size_t i = 0; i < n; ++i) {
        uv[2 * i] = ts.tracks[i].feature_points[0].u;
        uv[2 * i + 1] = ts.tracks[i].feature_points[0].v;
        ground[i] = 0;
        for (int l : p.ground_labels) ground[i] |= ts.tracks[i].label == l;
    }
}

// The depths a driver assigned to the tracks of its sequence in the last frames (per track a ring, newest at head - 1).
// A frame may come here twice (announced to the depth thread, then handed to process() with another message for the same stamp, or
// announced and never processed): the statistics count a stamp once and the history REPLACES the entry of a stamp it already holds.
struct DepthHistory {
    // the statistics count this message's stamp (false: it was the last one recorded)
    bool counts(const Tracklets& ts) const { return !(counted_any_ && !ts.stamps.empty() && counted_stamp_ == ts.stamps.front()); }
    // Remembers this frame's depth per track (sweep_depth[i] where the sweep was used and the caller knew none, else the message's) and
    // fills the history points from the memory: the depth of EVERY point of every track, in message order, into `out`.
    void record(const Tracklets& ts, const float* sweep_depth /* [tracks] or null */, std::vector<float>& out, int& features_with_depth) {
        const size_t n = ts.tracks.size();
        const bool counted = !counts(ts);
        const TimestampNSec stamp = ts.stamps.front();
        out.clear();
        for (size_t i = 0; i < n; ++i) {
            const Tracklet& tr = ts.tracks[i];
            if (tr.feature_points.empty()) continue;
            const float d0 = (sweep_depth && tr.feature_points[0].d < 0.f) ? sweep_depth[i] : tr.feature_points[0].d;  // (a depth the caller knows stays)
            out.push_back(d0);
            History& h = history_[tr.id];
            if (h.n > 0 && h.stamp[(h.head - 1) & (History::kDepth - 1)] == stamp) {
                h.d[(h.head - 1) & (History::kDepth - 1)] = d0;
            } else {
                h.stamp[h.head] = stamp;
                h.d[h.head] = d0;
                h.head = (h.head + 1) & (History::kDepth - 1);
                h.n = std::min<int>(History::kDepth, h.n + 1);
            }
            for (size_t k = 1; k < tr.feature_points.size(); ++k) {
                float dk = tr.feature_points[k].d;
                if (dk < 0.f && k < ts.stamps.size()) {
                    // (a track seen in consecutive frames has the entry of stamps[k] k places behind the newest: looked at first; stamps
                    // are unique inside a history, so the scan finds the same entry or none)
                    const int e = (h.head - 1 - (int)k) & (History::kDepth - 1);
                    if ((int)k < h.n && h.stamp[e] == ts.stamps[k]) {
                        dk = h.d[e];
                    } else {
                        for (int j = 0; j < h.n; ++j) {
                            const int e2 = (h.head - 1 - j) & (History::kDepth - 1);
                            if (h.stamp[e2] == ts.stamps[k]) dk = h.d[e2];
                        }
                    }
                }
                out.push_back(dk);
            }
            if (!counted) features_with_depth += d0 > 0.f;
        }
        counted_any_ = true;
        counted_stamp_ = stamp;
    }
    void forgetEndedTracks(const Tracklets& ts) {  // every 64 frames
        if (++frames_since_gc_ < 64) return;
        frames_since_gc_ = 0;
        const TimestampNSec oldest = ts.stamps.back();
        for (auto it = history_.begin(); it != history_.end();)
            it = it->second.stamp[(it->second.head - 1) & (History::kDepth - 1)] < oldest ? history_.erase(it) : std::next(it);
    }

private:
    struct History {
        static constexpr int kDepth = 16;
        TimestampNSec stamp[kDepth];
        float d[kDepth];
        int head = 0, n = 0;
    };
    std::unordered_map<unsigned long, History> history_;
    int frames_since_gc_ = 0;
    TimestampNSec counted_stamp_ = 0;  // the last frame whose features went into the statistics (record is idempotent per stamp)
    bool counted_any_ = false;
};

inline void applyDepths(Tracklets& ts, const std::vector<float>& d) {
    size_t j = 0;
    for (auto& tr : ts.tracks)
        for (auto& fp : tr.feature_points) fp.d = d[j++];
}

// a product of estimated transforms: back onto SO(3) (convert() does not normalise, definitions.cpp:14-28)
inline EigenPose normalisedPrior(const EigenPose& prior) {
    Pose q = convert(prior);
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= n;
    return convert(q);
}

// the last frame's pose and motion of a sequence: the constant-velocity prior, and what every frame leaves behind
struct MotionState {
    EigenPose last_pose = EigenPose::Identity(), last_motion = EigenPose::Identity();
    bool have_last = false, have_motion = false;
    TimestampNSec last_stamp = 0;
    // constant velocity from the last two poses; before there are two: straight ahead at prior_speed
    EigenPose constantVelocityPrior(const StreamParams& p, TimestampNSec stamp) const {
        if (have_motion) return last_motion * last_pose;
        EigenPose m = EigenPose::Identity();
        m.t[0] = -p.prior_speed * (convert(stamp) - convert(last_stamp));  // new vehicle <- old vehicle
        return m * last_pose;
    }
    void advance(const EigenPose& pose, TimestampNSec stamp) {
        if (have_last) last_motion = pose * last_pose.inverse();
        have_motion = have_last;
        last_pose = pose;
        last_stamp = stamp;
        have_last = true;
    }
};

// five_point::motionUnscaled (five_point.hpp:650-671, helpers::getMotionUnscaled, general_helpers.hpp:209-231) in three steps, so that
// the estimator of its middle line can be the host's, limo_five_point or one frame of limo_five_point_batch: matches and the mean-flow
// gate (fivePointQuery), the estimate (query.estimate says whether one is wanted), the scaling by speed x dt and the frame changes
// (fivePointUnscaled).
struct FivePointQuery {
    std::vector<Vector2d> last_points, cur_points;
    EigenPose cam_t0_t1 = EigenPose::Identity();  // camera at t0 <- camera at t1: what stands without an estimate
    bool estimate = false;
};
inline void fivePointQuery(const Tracklets& tracklets, TimestampNSec stamp_last_kf, TimestampNSec stamp_cur, FivePointQuery& q) {
    q.last_points.clear(), q.cur_points.clear();
    five_point::matches(tracklets, stamp_last_kf, stamp_cur, {23, 24, 25, 26}, q.last_points, q.cur_points);
    q.cam_t0_t1 = EigenPose::Identity();
    q.cam_t0_t1.t[2] = 1.;
    q.estimate = !q.last_points.empty() && five_point::meanFlow(q.last_points, q.cur_points) >= 5.;
    if (!q.estimate && !q.last_points.empty()) q.cam_t0_t1.t[2] = 0.;  // "not enough flow": calcMotion5Point zeroes the translation before it returns (:118-121)
}
// (calcMotion5Point: findEssentialMat(points1 = cur, points0 = last), recoverPose(E, cur, last): x_last = R x_cur + t)
inline five_point::Motion fivePointOnHost(const FivePointQuery& q, const Camera& camera, uint64_t seed) {
    return five_point::estimateMotion(q.cur_points, q.last_points, camera.focal_length, camera.principal_point, 0.999, 2.0, seed);
}
inline limo_five_point_frame fivePointFrame(const FivePointQuery& q, uint64_t seed) {
    static_assert(sizeof(Vector2d) == 2 * sizeof(double), "Vector2d is two doubles: a point list is the [n*2] array of the C-ABI");
    limo_five_point_frame fr;
    fr.n = (int32_t)std::min(q.cur_points.size(), q.last_points.size());
    fr.pts_a = fr.n ? &q.cur_points[0].v[0] : nullptr;
    fr.pts_b = fr.n ? &q.last_points[0].v[0] : nullptr;
    fr.seed = seed;
    return fr;
}
inline five_point::Motion fivePointMotion(const limo_five_point_motion& mo) {
    five_point::Motion m;
    m.ok = mo.ok != 0;
    m.inliers = mo.inliers;
    m.in_front = mo.in_front;
    m.samples = mo.samples;
    for (int i = 0; i < 9; ++i) {
        m.E[i] = mo.E[i];
        m.R[i] = mo.R[i];
    }
    for (int i = 0; i < 3; ++i) m.t[i] = mo.t[i];
    return m;
}
inline EigenPose fivePointUnscaled(const StreamParams& p, const Camera& camera, const FivePointQuery& q, const five_point::Motion* m, TimestampNSec stamp_last_kf,
                                   TimestampNSec stamp_cur) {
    EigenPose cam_t0_t1 = q.cam_t0_t1;
    if (m && m->ok) {
        for (int i = 0; i < 9; ++i) cam_t0_t1.R[i] = m->R[i];
        for (int i = 0; i < 3; ++i) cam_t0_t1.t[i] = m->t[i];
    }
    const double dt = convert(stamp_cur) - convert(stamp_last_kf);
    const double n = std::sqrt(cam_t0_t1.t[0] * cam_t0_t1.t[0] + cam_t0_t1.t[1] * cam_t0_t1.t[1] + cam_t0_t1.t[2] * cam_t0_t1.t[2]);
    for (int i = 0; i < 3; ++i) cam_t0_t1.t[i] = cam_t0_t1.t[i] / std::max(0.0001, n) * p.prior_speed * dt;
    const EigenPose T_camera_vehicle = camera.getEigenPose();
    return T_camera_vehicle.inverse() * cam_t0_t1.inverse() * T_camera_vehicle;
}
// mono_lidar.cpp:157-186: the unscaled motion since the last keyframe gets the length speed of the last two keyframes x time since the
// last one (prior_speed, already applied, while there is only one keyframe) and is applied to the last keyframe's pose.
inline EigenPose fivePointPrior(const BundleAdjusterKeyframes& ba, TimestampNSec stamp, EigenPose motion) {
    const Keyframe& last_kf = ba.getKeyframe();
    const auto kfs = ba.getSortedActiveKeyframePtrs();
    if (kfs.size() > 1) {
        const Keyframe &k1 = *kfs[kfs.size() - 1], &k0 = *kfs[kfs.size() - 2];
        const double speed = (k1.getEigenPose() * k0.getEigenPose().inverse()).translation().norm() / (convert(k1.timestamp_) - convert(k0.timestamp_));
        const double n = std::sqrt(motion.t[0] * motion.t[0] + motion.t[1] * motion.t[1] + motion.t[2] * motion.t[2]);
        for (int i = 0; i < 3; ++i) motion.t[i] = motion.t[i] / std::max(0.0001, n) * speed * (convert(stamp) - convert(k1.timestamp_));
    }
    return motion * (kfs.empty() ? last_kf.getEigenPose() : kfs.back()->getEigenPose());
}

// bundle adjustment every time_between_keyframes, whether or not THIS frame became a keyframe (:245-246)
inline bool solveDue(const StreamParams& p, const BundleAdjusterKeyframes& ba, double now_sec, double last_solved_sec) {
    return ba.keyframes_.size() > 2 && now_sec - last_solved_sec > 0.98 * p.time_between_keyframes_sec;
}

// LIMO_STREAM_TRACE=1: one line per adjustPoseOnly / solve with the resulting pose at full precision (two drives on
// different back ends are compared call by call with it)
inline void trace(const BundleAdjusterKeyframes& ba, const char* what, TimestampNSec stamp, const Pose& p, double cost) {
    static const bool on = std::getenv("LIMO_STREAM_TRACE") != nullptr;
    if (on) {
        uint64_t h = 1469598103934665603ull;  // FNV-1a over the selected ids: two drives select the same SET iff the hashes agree
        for (const auto& id : ba.selected_landmark_ids_) h = (h ^ (uint64_t)id) * 1099511628211ull;
        std::fprintf(stderr, "trace %s %llu cost %.17g pose %.17g %.17g %.17g %.17g %.17g %.17g %.17g selected %zu set %016llx\n", what,
                     (unsigned long long)stamp, cost, p[0], p[1], p[2], p[3], p[4], p[5], p[6], ba.selected_landmark_ids_.size(), (unsigned long long)h);
    }
}

// One sequence: its adjuster, keyframe selector, depth history, motion state, statistics and pose list, the staging buffers and jobs of
// its device calls, and the frame in flight.  The host phases of a frame are the member functions below, in the order a frame runs
// them; after a phase the wants...() queries and the jobs say which call the driver owes the sequence before the next phase.  No phase
// touches a limo_ctx: phases of different sequences may run on different threads while one thread makes the calls.
struct Sequence {
    // five_point_device: the driver has a device call for the five-point estimates (else the host estimator runs inside choosePrior)
    Sequence(const StreamParams& params, Camera::Ptr cam, bool five_point_device, int dump_tag = -1)
            : p(params), camera(std::move(cam)), five_point_device_(five_point_device) {
        ba.dump_tag_ = dump_tag;
        configureSequence(p, ba, selector);
    }

    // ---- 1. a frame arrives.  The message is taken over (stamps[0] = this frame, every track's feature_points[0] = its point in this
    // frame); its depths are filled in by the depth functions below.
    void take(Tracklets&& message, const float* cloud_xyzi, size_t n_points, const EigenPose* external_prior) {
        tracklets = std::move(message);
        cloud = cloud_xyzi, n_pts = n_points;
        has_external = external_prior != nullptr;
        if (has_external) prior = *external_prior;
        stamp = tracklets.stamps.front();
        first = is_keyframe = solve_due = false;
        frame_cov = BundleAdjusterKeyframes::PoseCovariance();
        five_point_query.estimate = false;
    }

    // ---- the depth assignment of a message: stageFeatures, the driver's sweep call over depthFrame's arrays, recordDepths.  They take the
    // message by reference: the single driver's depth thread runs them on the NEXT frame's message, which the caller still holds.
    bool fromSweep(const Tracklets& ts, const float* cloud_xyzi, size_t n_points) const { return p.assign_depth && cloud_xyzi && n_points && !ts.tracks.empty(); }
    void stageFeatures(const Tracklets& ts) {
        depth.assign(ts.tracks.size(), -1.f);
        stream_detail::stageFeatures(p, ts, uv, ground);
    }
    limo_depth_frame depthFrame(const Tracklets& ts, const float* cloud_xyzi, size_t n_points) { return {cloud_xyzi, n_points, uv.data(), ts.tracks.size(), ground.data(), depth.data()}; }
    // remembers this frame's depth per track and fills the history points from the memory (ring of the last frames): point_d
    void recordDepths(const Tracklets& ts, bool from_sweep) {
        if (history.counts(ts)) stats.features += (int)ts.tracks.size();
        timed(stats.sec_depth_history, [&] { history.record(ts, from_sweep ? depth.data() : nullptr, point_d, stats.features_with_depth); });
        history.forgetEndedTracks(ts);
    }
    // ... and for the frame in flight
    bool wantsSweep() const { return fromSweep(tracklets, cloud, n_pts); }
    void stageDepth() {
        if (wantsSweep()) stageFeatures(tracklets);
    }
    void recordDepth() { recordDepths(tracklets, wantsSweep()); }
    void applyDepths() { stream_detail::applyDepths(tracklets, point_d); }  // point_d (recordDepths of this message) into the message

    // ---- 2. with the depths in the message.  The first frame of a sequence is a Pose-fixed keyframe at the origin (:305-326): it is
    // handed over here.  A later frame gets its prior: the caller's, the five-point prior (the matches and the flow gate here; the estimate
    // by the driver's device call where wantsFivePoint(), else by the host estimator here) or constant velocity.
    void choosePrior() {
        first = ba.keyframes_.empty();
        pose = EigenPose::Identity();
        if (first) {
            cur = makeKeyframe(EigenPose::Identity(), Keyframe::FixationStatus::Pose);
            handOver();
        } else if (has_external) {
        } else if (p.motion_prior == StreamParams::MotionPrior::FivePoint) {
            stamp_last_kf = ba.getKeyframe().timestamp_;
            fivePointQuery(tracklets, stamp_last_kf, stamp, five_point_query);
            if (five_point_query.estimate) {
                ++stats.five_point_calls;
                if (!five_point_device_) last_five_point = timed(stats.sec_five_point, [&] { return fivePointOnHost(five_point_query, *camera, (uint64_t)stamp); });
            }
        } else {
            prior = motion.constantVelocityPrior(p, stamp);
        }
    }
    bool wantsFivePoint() const { return five_point_query.estimate && five_point_device_; }
    bool estimatedOnHost() const { return five_point_query.estimate && !five_point_device_; }
    limo_five_point_frame fivePointFrame() const { return stream_detail::fivePointFrame(five_point_query, (uint64_t)stamp); }
    void acceptFivePoint(const limo_five_point_motion& mo) {
        last_five_point = fivePointMotion(mo);
        ++stats.five_point_device_calls;
    }

    // ---- 3. Keyframe(prior) (:192-211).  mono_lidar.cpp:157-186 for the five-point prior: direction of the motion since the last keyframe
    // (straight ahead when the image flow is too small for an estimate), length = speed of the last two keyframes x time since the last
    // one (prior_speed while there is only one keyframe), applied to the last keyframe's pose.
    void buildKeyframe() {
        if (first) return;
        if (!has_external && p.motion_prior == StreamParams::MotionPrior::FivePoint) {
            const EigenPose unscaled = fivePointUnscaled(p, *camera, five_point_query, five_point_query.estimate ? &last_five_point : nullptr, stamp_last_kf, stamp);
            prior = fivePointPrior(ba, stamp, unscaled);
        }
        prior = normalisedPrior(prior);
        cur = timed(stats.sec_keyframe, [&] { return makeKeyframe(prior, Keyframe::FixationStatus::None); });
        if (wantsPoseOnly()) timed(stats.sec_pose_only, [&] { ba.preparePoseOnly(*cur, pose_job); });
    }
    // a prior without scale is always refined against the fixed landmarks of the last selection (:200-211; before the first solve() that
    // selection is empty); a frame with an external prior is not
    bool wantsPoseOnly() const { return !first && !has_external; }

    // ---- 4. the refined pose, keyframe selection (:218-222); a selected frame is handed over (:231-233)
    void selectKeyframe() {
        if (first) return;
        if (wantsPoseOnly()) {
            timed(stats.sec_pose_only, [&] { ba.commitPoseOnly(pose_job); });
            stats.sec_abi_pose_only += ba.last_report_.time_sec;
            if (p.pose_covariance) frame_cov = ba.lastPoseCovariance(stamp);
            trace("pose-only", cur->pose_);
        }
        pose = cur->getEigenPose();
        const auto selected = timed(stats.sec_select, [&] { return selector.select({cur}, ba.getActiveKeyframePtrs()); });
        if (selected.empty()) return;
        if (selected.size() != 1 || *selected.begin() != cur) throw std::logic_error("the keyframe selector returned a frame it was not given");
        handOver();
    }
    bool wantsPush() const { return push.kf != nullptr; }  // push: the job of limo_landmark_init (no landmark in it: no call)

    // ---- 5. the keyframe's landmarks enter the window.  Bundle adjustment every time_between_keyframes, whether or not THIS frame became a
    // keyframe (:245-263): window cut, labels, and the selection prepared - made here where the host selector makes it.
    void enterWindow() {
        if (wantsPush()) {
            Timed t(stats.sec_push);
            ba.commitPush(push);
            push.kf.reset();
        }
        if (first || !solveDue(p, ba, convert(stamp), last_solved_sec)) return;
        solve_due = true;
        {
            Timed t(stats.sec_window);
            const auto t0 = std::chrono::steady_clock::now();
            ba.deactivateKeyframes(p.min_number_connecting_landmarks, 3, p.max_size_optimization_window);
            const auto t1 = std::chrono::steady_clock::now();
            ba.updateLabels(tracklets, p.shrubbery_weight);
            if (std::getenv("LIMO_SHIM_TRACE"))
                std::fprintf(stderr, "[shim] window cut %.0f us, labels %.0f us\n", std::chrono::duration<double, std::micro>(t1 - t0).count(),
                             std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count());
        }
        timed(stats.sec_solve, [&] { ba.prepareSelection(select); });
        if (!wantsSelection()) selectionDone(false);
    }
    bool wantsSelection() const { return solve_due && select.on_device; }  // select: a pool for limo_landmark_select
    // ok: the device made the selection (else the host selector makes it here); the window of the solve is flattened
    void selectionDone(bool ok) {
        Timed t(stats.sec_solve);
        ba.commitSelection(select, ok);
        ba.prepareSolve(solve_job);
    }
    bool wantsSolve() const { return solve_due; }  // solve_job: the window for limo_ba_solve

    // ---- 6. the solved window, the pose of the frame (:281-294), what the frame leaves behind.  Returns the pose (keyframe <- origin).
    const EigenPose& finishFrame() {
        if (solve_due) {
            last_summary = timed(stats.sec_solve, [&] { return ba.commitSolve(solve_job); });
            stats.sec_abi_solve += ba.last_report_.time_sec;
            ++stats.solves;
            trace("solve", ba.getKeyframe().pose_);
            stats.solves_on_non_keyframes += !is_keyframe;
            last_solved_sec = convert(stamp);
        }
        // the optimised pose if the frame became a keyframe, its prior otherwise
        if (!first && ba.getKeyframe().timestamp_ == stamp) pose = ba.getKeyframe().getEigenPose();
        motion.advance(pose, stamp);
        ++stats.frames;
        stats.keyframes += is_keyframe;
        poses.push_back(pose);
        if (p.pose_covariance) covariances.push_back(frame_cov);
        cur.reset();
        pose_job.flat.reset(), solve_job.flat.reset(), select.flat.reset();
        return poses.back();
    }

    // KITTI odometry rows of the frames so far (helpers::poseToString, mono_lidar.cpp:281-294): camera_0 <- camera_t of every pose
    void writeKittiTrajectory(std::ostream& os) const {
        const EigenPose cv = camera->getEigenPose();
        for (const auto& pose_kf_origin : poses) kitti_io::writePoseRow(os, kitti_io::inCameraFrame(cv, pose_kf_origin.inverse()));
    }

    // StreamParams::pose_covariance: one row per frame so far - the 36 numbers of the covariance of the frame's adjustPoseOnly (tangent
    // units of limo_hip.h, %.17g) and its status; a frame that was not refined (the first, one with an external prior) has zeros and
    // LIMO_COV_NOT_COMPUTED
    void writeCovariances(std::ostream& os) const {
        char buf[40];
        for (const auto& c : covariances) {
            for (double v : c.cov) {
                std::snprintf(buf, sizeof(buf), "%.17g ", v);
                os << buf;
            }
            os << c.status << "\n";
        }
    }

    const StreamParams& p;
    Camera::Ptr camera;
    BundleAdjusterKeyframes ba;
    KeyframeSelector selector;
    DepthHistory history;  // the depths this sequence's tracks were assigned in the last frames they were seen in
    MotionState motion;
    StreamStats stats;
    std::vector<EigenPose> poses;
    std::vector<BundleAdjusterKeyframes::PoseCovariance> covariances;  // per frame, with StreamParams::pose_covariance
    BundleAdjusterKeyframes::PoseCovariance frame_cov;                // ... of the frame in flight
    std::string last_summary;
    five_point::Motion last_five_point;  // the last five-point estimate (diagnostics: inliers, samples)
    std::vector<float> uv, depth, point_d;  // staging of the sweep call, its result, the depth of every point of the message
    std::vector<uint8_t> ground;
    // the frame in flight
    Tracklets tracklets;
    const float* cloud = nullptr;
    size_t n_pts = 0;
    TimestampNSec stamp = 0;
    EigenPose pose;  // what the frame reports (keyframe <- origin)
    BundleAdjusterKeyframes::PushJob push;
    BundleAdjusterKeyframes::WindowJob pose_job, solve_job;
    BundleAdjusterKeyframes::SelectJob select;

private:
    // (this sequence owns its keyframes and never edits their measurements_: the table is built once per keyframe and kept for its life
    // in the window)
    Keyframe::Ptr makeKeyframe(const EigenPose& at, Keyframe::FixationStatus fixation) const {
        Plane ground_plane;
        ground_plane.distance = p.height_over_ground;
        auto kf = std::make_shared<Keyframe>(stamp, tracklets, camera, at, fixation, ground_plane);
        kf->freezeMeasurements();
        return kf;
    }
    // the frame becomes a keyframe (its keyframe object is not looked at again: handed over instead of copying its maps)
    void handOver() {
        Timed t(stats.sec_push);
        ba.preparePush(std::move(*cur), push);
        is_keyframe = true;
    }
    void trace(const char* what, const Pose& at) const { stream_detail::trace(ba, what, stamp, at, ba.last_report_.final_cost); }

    const bool five_point_device_;
    bool has_external = false, first = false, is_keyframe = false, solve_due = false;
    EigenPose prior;
    TimestampNSec stamp_last_kf = 0;
    double last_solved_sec = -1e30;
    Keyframe::Ptr cur;
    FivePointQuery five_point_query;
};

}  // namespace stream_detail

}  // namespace keyframe_bundle_adjustment
