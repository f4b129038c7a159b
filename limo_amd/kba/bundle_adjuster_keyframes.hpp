// bundle_adjuster_keyframes.hpp — the reference's VO-backend class with the HIP library behind it.
//
// Same class name, method names, argument meaning, exceptions and PUBLIC DATA MEMBERS as
// keyframe_bundle_adjustment/include/keyframe_bundle_adjustment/bundle_adjuster_keyframes.hpp:40-335, so callers
// (mono_lidar.cpp:88-373, the gtests) keep working.  What changed: solve() / adjustPoseOnly() no longer build a
// ceres::Problem; they flatten the window and call limo_ba_solve / limo_ba_adjust_pose_only (include/limo_hip.h).
// Results are written back in place into Keyframe::pose_, Keyframe::local_ground_plane_, Landmark::pos.
#pragma once
#include <exception>
#include <string>

#include "keyframe.hpp"
#include "landmark_selector.hpp"

#include "../../include/limo_hip.h"  // limo_ctx, limo_ray, limo_ba_iteration

namespace keyframe_bundle_adjustment {

struct FlatWindow;  // a window flattened into the arrays of the C-ABI (bundle_adjuster_keyframes.cpp)

// For every caller of the C-ABI here (this shim, stream_driver.hpp, lockstep_driver.hpp).  createContext: a context on the GPU that
// LIMO_DEVICE names (default 0: one process per GPU, scripts/stream_replicas.py); throws where there is none - the hot path needs the
// HIP library and an MI355X, there is no CPU fallback.  checkCall: throws "<what>: <limo_last_error>" unless rc is LIMO_OK.
limo_ctx* createContext();
void checkCall(limo_ctx* ctx, int rc, const char* what);

class BundleAdjusterKeyframes {
public:
    using UPtr = std::unique_ptr<BundleAdjusterKeyframes>;
    using Ptr = std::shared_ptr<BundleAdjusterKeyframes>;

    struct NotEnoughKeyframesException : public std::exception {
        NotEnoughKeyframesException(size_t num_is, size_t num_should_be);
        const char* what() const noexcept override { return msg.c_str(); }
        size_t num_is;
        size_t num_should_be;
        std::string msg;  // (the reference returns a dangling c_str(); we keep the text alive)
    };
    struct KeyframeNotFoundException : public std::exception {
        explicit KeyframeNotFoundException(TimestampNSec timestamp);
        const char* what() const noexcept override { return msg.c_str(); }
        TimestampNSec ts_;
        std::string msg;
    };
    struct OutlierRejectionOptions {  // bundle_adjuster_keyframes.hpp:79-89
        double depth_thres{0.16};
        double reprojection_thres{1.6};
        double depth_quantile{0.95};
        double reprojection_quantile{0.95};
        int num_iterations{1};
    };

    BundleAdjusterKeyframes();
    ~BundleAdjusterKeyframes();
    BundleAdjusterKeyframes(const BundleAdjusterKeyframes&) = delete;
    BundleAdjusterKeyframes& operator=(const BundleAdjusterKeyframes&) = delete;

    void push(const Keyframe& kf);
    void push(Keyframe&& kf);  // (same, without copying the keyframe's measurement maps: for callers that hand the keyframe over)
    void push(const std::vector<Keyframe>& kfs);
    std::string solve();
    void deactivateKeyframes(int min_num_connecting_landmarks = 3, int min_size_optimization_window = 4,
                             int max_size_optimization_window = 20);
    const Keyframe& getKeyframe(TimestampSec timestamp = -1.) const;
    std::map<KeyframeId, Keyframe::Ptr> getActiveKeyframePtrs() const;
    std::map<KeyframeId, Keyframe::ConstPtr> getActiveKeyframeConstPtrs() const;
    std::vector<Keyframe::Ptr> getSortedActiveKeyframePtrs() const;
    std::vector<std::pair<KeyframeId, Keyframe::Ptr>> getSortedIdsWithActiveKeyframePtrs() const;
    std::map<LandmarkId, Landmark::ConstPtr> getActiveLandmarkConstPtrs() const;
    std::map<LandmarkId, Landmark::ConstPtr> getSelectedLandmarkConstPtrs() const;
    std::string adjustPoseOnly(Keyframe&);
    bool calculateLandmark(const Keyframe& kf, const LandmarkId& lId, Vector3d& posAbs);
    bool calculateLandmark(const LandmarkId& lId, Vector3d& posAbs);
    void set_solver_time(double solver_time_sec);
    void updateLabels(const Tracklets& t, double shrubbery_weight = 1.);

    // numbers behind the last report string (not in the reference; handy for tests and drivers)
    struct LastReport {
        int termination = -1, num_solves = 0, iterations_total = 0, n_trimmed_landmarks = 0;
        int n_depth_blocks = 0, n_repr_blocks = 0, n_gp_blocks = 0;
        double initial_cost = 0, final_cost = 0, time_sec = 0;
    } last_report_;

    // Ceres' per-iteration progress table (the reference sets Solver::Options::minimizer_progress_to_stdout = true,
    // robust_optimization/robust_solving.hpp:105; off here by default - this shim has printed nothing so far).  true: solve() and
    // adjustPoseOnly() switch the library's iteration log on (include/limo_hip.h:limo_ba_iteration), keep the entries of their call
    // (lastIterations) and print to stdout: a caption line per call, then one header and one row per entry for every solve of the
    // schedule.  A backend without the
    // iteration-log symbols gives no log: nothing is printed, lastIterations() is empty.
    bool minimizer_progress_to_stdout_ = false;
    const std::vector<limo_ba_iteration>& lastIterations() const {
        return last_iterations_;
    }

    // Marginal covariance of the poses a call returns (not in the reference; include/limo_hip.h, "Pose covariance": what
    // ceres::Covariance::GetCovarianceBlockInTangentSpace gives for a pose block of the problem just solved).  setPoseCovariance(true):
    // solve() and adjustPoseOnly() switch the library's pass on and keep, for every keyframe of their window, the 6 x 6 block
    // (rotation 3 | translation 3, row-major, the solve's tangent units: the rotation tangent is a left-multiplied HALF-angle vector)
    // and the window's status; lastPoseCovariance(id) reads the last call's.  A keyframe the last call did not hold, the switch off
    // and a backend without the symbols give LIMO_COV_NOT_COMPUTED and zeros.
    struct PoseCovariance {
        std::array<double, 36> cov{};
        int status = LIMO_COV_NOT_COMPUTED;
    };
    void setPoseCovariance(bool on) { pose_covariance_ = on; }
    bool poseCovariance() const { return pose_covariance_; }
    PoseCovariance lastPoseCovariance(KeyframeId id) const {
        const auto it = last_pose_cov_.find(id);
        return it == last_pose_cov_.end() ? PoseCovariance() : it->second;
    }
    // ... in rotation-vector units: the rotation rows and columns times 2
    static void toRotationVectorUnits(std::array<double, 36>& c) {
        for (int i = 0; i < 36; ++i) c[i] *= (i / 6 < 3 ? 2. : 1.) * (i % 6 < 3 ? 2. : 1.);
    }

    // Where solve() selects its landmarks (not in the reference).  With parameters set, solve() flattens the active landmarks, minus the
    // selector's outliers, into a limo_select_pool and calls limo_landmark_select (the device form of cheirality + voxel + add-depth as
    // StreamDriver wires them: include/limo_hip.h); the selector takes the result over (LandmarkSelector::acceptSelection), so outliers,
    // categories and the unselected bookkeeping go on as before.  landmark_selector_->select runs instead whenever the call returns
    // anything but LIMO_OK (a window above 64 keyframes or 8 cameras, a backend without the symbol).  The parameters must say what the
    // schemes added to landmark_selector_ say: the two paths then give the same selection.  nullptr turns it off; off is the default.
    void setDeviceSelection(const limo_select_params* params);
    int device_selections_ = 0;  // solve() calls whose selection limo_landmark_select made

    // Split-phase forms of push, adjustPoseOnly, the selection in front of solve and solve (not in the reference).  Each method above is
    // prepare + run + commit.  run... makes the job's ONE C-ABI call on this adjuster's own context, with all that belongs to the call:
    // the iteration log, the exceptions, the host selector where the device refuses the pool.  A caller that drives several adjusters
    // in lock step (lockstep_driver.hpp) prepares them all, makes one batched call over the jobs in place of the run... pieces
    // (limo_landmark_init over the concatenated rays, limo_ba_adjust_pose_only_batch, limo_landmark_select_batch, limo_ba_batch_create /
    // _solve / _download), checks its return code and commits each.  A job owns every buffer its C-ABI arguments point into; prepare
    // and commit never touch a limo_ctx, so adjusters of different sequences may be prepared and committed on different threads while one
    // thread makes the calls.
    struct PushJob {  // limo_landmark_init(ids.size(), off, rays, use_depth, pos, ok); ids.empty(): no call
        Keyframe::Ptr kf;
        std::vector<LandmarkId> ids;
        std::vector<int32_t> off{0};
        std::vector<limo_ray> rays;
        std::vector<uint8_t> use_depth;
        std::vector<double> pos;   // [3 * ids.size()]  result
        std::vector<uint8_t> ok;   // [ids.size()]      result
    };
    void preparePush(Keyframe&& kf, PushJob& job);
    void runPush(PushJob& job);
    void commitPush(PushJob& job);
    struct WindowJob {  // limo_ba_adjust_pose_only(window, has_prior ? &prior : NULL, &opts, &report) / limo_ba_solve(window, &opts, &report)
        std::shared_ptr<FlatWindow> flat;  // the buffers behind `window`
        limo_ba_window* window = nullptr;
        limo_speed_prior prior{};
        bool has_prior = false;
        limo_ba_options opts{};
        limo_ba_report report{};           // result
        // result, with setPoseCovariance(true): the window's [6 n_kf][6 n_kf] matrix and status (whoever makes the call fills them:
        // run..., or the lock-step driver from limo_ctx_last_pose_covariance of its batched call); commit... keeps the keyframes' blocks
        std::vector<double> cov;
        int32_t cov_status = LIMO_COV_NOT_COMPUTED;
    };
    void preparePoseOnly(Keyframe& kf, WindowJob& job);
    void runPoseOnly(WindowJob& job);
    std::string commitPoseOnly(WindowJob& job);
    struct SelectJob {  // on_device: limo_landmark_select(&pool, params, out.data()); else there is nothing to call
        LandmarkView active_lms;
        std::map<KeyframeId, Keyframe::ConstPtr> active_kfs;
        bool on_device = false;
        std::shared_ptr<FlatWindow> flat;  // the buffers behind `pool`, with the three below
        std::vector<uint64_t> kf_stamp, lm_id;
        std::vector<uint8_t> has_depth;
        limo_select_pool pool{};
        const limo_select_params* params = nullptr;  // (this adjuster's: valid until its next setDeviceSelection)
        std::vector<uint8_t> out;          // result
    };
    void prepareSelection(SelectJob& job);                   // throws NotEnoughKeyframesException as solve() does
    bool runSelection(SelectJob& job);                       // the device made the selection: commitSelection's device_ok
    void commitSelection(SelectJob& job, bool device_ok);    // device_ok = false: the host selector runs
    void prepareSolve(WindowJob& job);                       // (after commitSelection: flattens selected_landmark_ids_)
    void runSolve(WindowJob& job);                           // throws NotEnoughKeyframesException as solve() does
    std::string commitSolve(WindowJob& job);
    // LIMO_KBA_DUMP files of this adjuster are named solve_sII_NNNNNN.bin with II = dump_tag_ and its own count (>= 0: a sequence of a
    // lock-step drive); -1: solve_NNNNNN.bin, counted over the process as before
    int dump_tag_ = -1;

public:
    std::map<KeyframeId, Keyframe::Ptr> keyframes_;
    std::map<LandmarkId, Landmark::Ptr> landmarks_;
    std::set<KeyframeId> active_keyframe_ids_;
    std::set<LandmarkId> active_landmark_ids_;
    std::set<LandmarkId> selected_landmark_ids_;
    OutlierRejectionOptions outlier_rejection_options_;
    std::unique_ptr<LandmarkSelector> landmark_selector_;
    // cityscapes labels, bundle_adjuster_keyframes.hpp:229-255
    std::map<std::string, std::set<int>> labels_{{"outliers", {23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33}},
                                                 {"shrubbery", {21}},
                                                 {"ground", {6, 7, 8, 9, 10}}};

private:
    std::map<LandmarkId, Landmark::ConstPtr> filterLandmarksById(const std::set<LandmarkId>& ids) const;
    void collectRays(const Keyframe& kf, const LandmarkId& lId, std::vector<limo_ray>& rays) const;  // this keyframe's views
    void collectRays(const LandmarkId& lId, std::vector<limo_ray>& rays) const;                      // every active keyframe
    limo_ctx* context();
    // landmark ids a pushed keyframe measures, in id order (the keys of its measurements_ as one contiguous array: the window cut
    // merges them instead of walking the maps node by node); rebuilt from the map whenever it does not look like it any more
    const std::vector<LandmarkId>& measuredIds(const Keyframe& kf);
    void setIterationLog(limo_ctx* ctx);      // before the solve: the context's switch follows minimizer_progress_to_stdout_
    void collectIterations(limo_ctx* ctx, const char* what);  // behind it: last_iterations_ and the table
    std::vector<limo_ba_iteration> last_iterations_;
    void setCovarianceSwitch(limo_ctx* ctx, WindowJob& job);   // before the call: the context's switch follows pose_covariance_
    void collectCovariance(limo_ctx* ctx, WindowJob& job);     // behind it: window 0 of the call into job.cov / job.cov_status
    void keepCovariance(const WindowJob& job);                 // commit...: last_pose_cov_ from the job
    bool pose_covariance_ = false;
    std::map<KeyframeId, PoseCovariance> last_pose_cov_;
    // LIMO_SHIM_TRACE=1: where the host time of adjustPoseOnly() / solve() goes.  Every half and piece adds its microseconds here;
    // commitPoseOnly / commitSolve print the line and start over (a call somebody else made, a batched one, shows as 0 us).
    struct ShimTimes {
        double select = 0., prepare = 0., call = 0.;
    } shim_us_;
    int dump_calls_ = 0;
    bool device_selection_ = false;
    limo_select_params select_params_{};
    std::vector<limo_select_add> select_add_;
    limo_ctx* ctx_ = nullptr;
    double solver_time_sec;
};

}  // namespace keyframe_bundle_adjustment
