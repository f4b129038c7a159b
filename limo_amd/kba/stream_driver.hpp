// stream_driver.hpp — ROS-free streaming driver of ONE sequence on the MI355X library.  What a frame does is stream_detail::Sequence's
// (sequence.hpp: the call order of the reference's node, as host phases); process() runs those phases and makes, between them, one
// device call each: limo_depth_estimate on this driver's context, the five-point estimate on a context of its own, the adjuster's
// run... pieces (bundle_adjuster_keyframes.hpp) on the adjuster's.  What is this driver's alone: the depth assignment one frame ahead
// of the bundle adjuster (StreamParams::DepthAhead: a thread, or begin / end on its own stream), and the timing of the stages.
// N sequences of one rig at once: lockstep_driver.hpp (the same phases, one batched call per stage).
#pragma once
#include <condition_variable>
#include <mutex>
#include <thread>

#include "sequence.hpp"

// The five-point entry points are weak references: the driver also links against backends that serve the C-ABI without them (the
// test backends tests/cpp/oracle_abi.cpp and emu_pipeline.cpp) - there the addresses are null and the host estimator runs.
#pragma weak limo_five_point
#pragma weak limo_five_point_default_params

namespace keyframe_bundle_adjustment {

class StreamDriver {
public:
    using Stats = StreamStats;

    StreamDriver(const StreamParams& p, Camera::Ptr camera, const EigenPose& T_camera_lidar)
            : p_(p), T_cam_lidar_(convert(T_camera_lidar)),
              seq_(p_, camera, p.five_point_on_device && &limo_five_point != nullptr && &limo_five_point_default_params != nullptr), ctx_(createContext()) {
        limo_depth_default_params(&depth_params_);
    }
    ~StreamDriver() {
        try {
            cancelPrefetch();
        } catch (...) {  // (an error of a depth job nobody picked up)
        }
        if (worker_.joinable()) {
            {
                std::lock_guard<std::mutex> lk(job_mutex_);
                job_state_ = JobState::Exit;
            }
            job_cv_.notify_all();
            worker_.join();
        }
        if (ctx_) limo_ctx_destroy(ctx_);
        if (five_point_ctx_) limo_ctx_destroy(five_point_ctx_);
    }
    StreamDriver(const StreamDriver&) = delete;
    StreamDriver& operator=(const StreamDriver&) = delete;

    // Start the depth assignment of a frame that process() will be given LATER (normally the next one): copies and kernels go onto
    // the stream of this driver's own context and run while the host thread and the bundle adjuster's context work on the current
    // frame - the reference's depth estimator is a process of its own beside the BA node (kitti_standalone.launch:14-23, :55).
    // `cloud_xyzi` must stay valid until that process() call (page-locked memory from limo_host_alloc makes the copy a DMA).
    // process() recognises the frame by its stamp and feature count; a prefetch that is not picked up is dropped.  Results are
    // those of the unprefetched call, bit for bit.
    void prefetchDepth(const Tracklets& tracklets, const float* cloud_xyzi, size_t n_pts) {
        if (!seq_.fromSweep(tracklets, cloud_xyzi, n_pts) || tracklets.stamps.empty()) return;
        stream_detail::Timed t(seq_.stats.sec_depth);
        closeOpenDepthCall();
        seq_.stageFeatures(tracklets);
        const Camera& cam = *seq_.camera;
        checkCall(ctx_,
                  limo_depth_estimate_begin(ctx_, cloud_xyzi, n_pts, T_cam_lidar_.data(), cam.focal_length, cam.principal_point[0], cam.principal_point[1], p_.image_width,
                                            p_.image_height, seq_.uv.data(), tracklets.tracks.size(), seq_.ground.data(), &depth_params_),
                  "limo_depth_estimate_begin");
        prefetch_open_ = true;
        prefetch_stamp_ = tracklets.stamps.front();
        prefetch_n_ = tracklets.tracks.size();
    }

    // The frame after the one the NEXT process() call is given: that call starts its depth assignment (StreamParams::depth_ahead)
    // as soon as it has finished its own - the depths of a track's older points come from the frames before, so the frames'
    // assignments run in order.  `tracklets` is the very object that will be handed to process() afterwards (an rvalue of it):
    // the depth thread reads it; it and the sweep must stay valid and untouched until then.
    void announceNextFrame(const Tracklets& tracklets, const float* cloud_xyzi, size_t n_pts) {
        next_tracklets_ = &tracklets;
        next_cloud_ = cloud_xyzi;
        next_n_pts_ = n_pts;
    }

    // Thread mode: returns when the depth thread has finished the frame it was given (a caller that times process() calls puts the
    // thread's work inside the timed region with it; process() waits by itself otherwise).
    void waitForDepthAhead() { waitForDepthThread(); }

    // Drop what prefetchDepth / announceNextFrame started (the sweep buffer is about to go away).
    void cancelPrefetch() {
        next_tracklets_ = nullptr;
        waitForDepthThread();
        ahead_valid_ = false;
        closeOpenDepthCall();
    }

    // One frame.  `tracklets`: the tracker's message - stamps[0] = this frame, every track's feature_points[0] = its point
    // in this frame (newest first).  Depths the caller already knows stay; the others (d < 0) are filled from the sweep:
    // point 0 by limo_depth_estimate on `cloud_xyzi` (KITTI velodyne layout, n_pts x 4 floats; may be null), points 1..
    // from what this driver assigned to the same track in earlier frames.  external_prior: keyframe <- origin pose of the
    // frame if the caller has one (the node's tf prior), else constant velocity.
    // Returns the frame's pose estimate (keyframe <- origin).
    EigenPose process(const Tracklets& message, const float* cloud_xyzi, size_t n_pts, const EigenPose* external_prior = nullptr) {
        return process(Tracklets(message), cloud_xyzi, n_pts, external_prior);
    }
    EigenPose process(Tracklets&& message, const float* cloud_xyzi, size_t n_pts, const EigenPose* external_prior = nullptr) {
        using clk = std::chrono::steady_clock;
        using stream_detail::timed;
        Stats& st = seq_.stats;
        const auto t_begin = clk::now();
        waitForDepthThread();  // (it may be writing into `message`)
        if (message.stamps.empty()) return seq_.motion.last_pose;  // (:98-104)
        seq_.take(std::move(message), cloud_xyzi, n_pts, external_prior);
        // what the depth thread prepared belongs to this message iff stamp, track count and point count agree (a copy of the announced
        // message is as good as the object itself; anything else is assigned here and the prepared depths are dropped)
        size_t n_points = 0;
        for (const auto& tr : seq_.tracklets.tracks) n_points += tr.feature_points.size();
        const bool depth_done = ahead_valid_ && ahead_stamp_ == seq_.stamp && ahead_tracks_ == seq_.tracklets.tracks.size() && seq_.point_d.size() == n_points;
        ahead_valid_ = false;
        if (depth_done)
            ++st.depth_prefetched;
        else
            computeDepths(seq_.tracklets, cloud_xyzi, n_pts);
        seq_.applyDepths();
        st.sec_depth += std::chrono::duration<double>(clk::now() - t_begin).count();
        if (next_tracklets_) {  // announceNextFrame
            const Tracklets* next = next_tracklets_;
            next_tracklets_ = nullptr;
            if (p_.depth_ahead == StreamParams::DepthAhead::Stream)
                prefetchDepth(*next, next_cloud_, next_n_pts_);
            else if (p_.depth_ahead == StreamParams::DepthAhead::Thread)
                startDepthThreadJob(next, next_cloud_, next_n_pts_);
        }
        // the phases of the frame (sequence.hpp); between them the call the sequence asks for, timed into the figure of its stage
        BundleAdjusterKeyframes& ba = seq_.ba;
        seq_.choosePrior();
        if (seq_.wantsFivePoint()) timed(st.sec_five_point, [&] { estimateFivePoint(); });
        seq_.buildKeyframe();
        if (seq_.wantsPoseOnly()) timed(st.sec_pose_only, [&] { ba.runPoseOnly(seq_.pose_job); });
        seq_.selectKeyframe();
        if (seq_.wantsPush()) timed(st.sec_push, [&] { ba.runPush(seq_.push); });
        seq_.enterWindow();
        if (seq_.wantsSelection()) seq_.selectionDone(timed(st.sec_solve, [&] { return ba.runSelection(seq_.select); }));
        if (seq_.wantsSolve()) timed(st.sec_solve, [&] { ba.runSolve(seq_.solve_job); });
        const EigenPose pose = seq_.finishFrame();
        st.sec_total += std::chrono::duration<double>(clk::now() - t_begin).count();
        return pose;
    }

    // KITTI odometry rows of the frames so far, 12 numbers per line (mono_lidar.cpp:281-294)
    void writeKittiTrajectory(std::ostream& os) const { seq_.writeKittiTrajectory(os); }
    void writeCovariances(std::ostream& os) const { seq_.writeCovariances(os); }  // (StreamParams::pose_covariance)

    BundleAdjusterKeyframes& adjuster() { return seq_.ba; }
    const std::vector<EigenPose>& poses() const { return seq_.poses; }
    const Stats& stats() const { return seq_.stats; }
    const five_point::Motion& lastFivePoint() const { return seq_.last_five_point; }
    const std::string& lastSummary() const { return seq_.last_summary; }
    limo_depth_params& depthParams() { return depth_params_; }

private:
    // limo_five_point with the arguments motionUnscaled gives estimateMotion (probability 0.999, 2 px, 1000 samples).  It runs on a
    // context of its own: the driver's first context belongs to the depth thread while a frame is in flight (DepthAhead::Thread).
    void estimateFivePoint() {
        if (!five_point_ctx_) five_point_ctx_ = createContext();
        limo_five_point_params prm;
        limo_five_point_default_params(&prm);
        const limo_five_point_frame fr = seq_.fivePointFrame();
        limo_five_point_motion mo;
        const Camera& cam = *seq_.camera;
        checkCall(five_point_ctx_, limo_five_point(five_point_ctx_, &fr, cam.focal_length, cam.principal_point[0], cam.principal_point[1], &prm, &mo, nullptr), "limo_five_point");
        seq_.acceptFivePoint(mo);
    }

    // ---- the depth thread (StreamParams::DepthAhead::Thread): one job at a time = computeDepths of the announced frame
    enum class JobState { Idle, Pending, Running, Exit };
    void startDepthThreadJob(const Tracklets* ts, const float* cloud, size_t n_pts) {
        if (!worker_.joinable()) worker_ = std::thread([this] { depthThreadMain(); });
        {
            std::lock_guard<std::mutex> lk(job_mutex_);
            job_ts_ = ts;
            job_cloud_ = cloud;
            job_n_pts_ = n_pts;
            job_error_ = nullptr;
            job_state_ = JobState::Pending;
        }
        job_cv_.notify_all();
    }
    // returns when no job is pending or running; a job that has finished leaves its frame's identity in ahead_* (its error is rethrown here)
    void waitForDepthThread() {
        if (!worker_.joinable()) return;
        std::unique_lock<std::mutex> lk(job_mutex_);
        job_cv_.wait(lk, [this] { return job_state_ == JobState::Idle; });
        if (job_ts_) {  // (the frame's identity was taken by the thread when it STARTED the job: the caller's message may be gone by now)
            ahead_valid_ = job_has_stamp_;
            ahead_stamp_ = job_stamp_;
            ahead_tracks_ = job_tracks_;
            job_ts_ = nullptr;
        }
        if (job_error_) {
            std::exception_ptr e = job_error_;
            job_error_ = nullptr;
            ahead_valid_ = false;
            std::rethrow_exception(e);
        }
    }
    void depthThreadMain() {
        std::unique_lock<std::mutex> lk(job_mutex_);
        for (;;) {
            job_cv_.wait(lk, [this] { return job_state_ == JobState::Pending || job_state_ == JobState::Exit; });
            if (job_state_ == JobState::Exit) return;
            job_state_ = JobState::Running;
            const Tracklets* ts = job_ts_;
            const float* cloud = job_cloud_;
            const size_t n_pts = job_n_pts_;
            job_has_stamp_ = !ts->stamps.empty();
            job_stamp_ = job_has_stamp_ ? ts->stamps.front() : 0;
            job_tracks_ = ts->tracks.size();
            lk.unlock();
            std::exception_ptr err;
            const auto t0 = std::chrono::steady_clock::now();
            try {
                if (!ts->stamps.empty()) computeDepths(*ts, cloud, n_pts);
            } catch (...) {
                err = std::current_exception();
            }
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            lk.lock();
            seq_.stats.sec_depth_thread += sec;
            job_error_ = err;
            if (job_state_ != JobState::Exit) job_state_ = JobState::Idle;
            job_cv_.notify_all();
        }
    }

    void closeOpenDepthCall() {  // a prefetch nobody will pick up: its limo_depth_estimate_end, results dropped
        if (!prefetch_open_) return;
        prefetch_open_ = false;
        std::vector<float> sink(prefetch_n_);
        (void)limo_depth_estimate_end(ctx_, sink.data(), prefetch_n_);
    }

    // The depths of a message: the newest point of every track from the sweep (limo_depth_estimate, or the end of the call prefetchDepth
    // began), the others from the history; all of them, in message order, into the sequence's point_d, which process() copies into
    // the message.  (The depth thread hands over that one contiguous array - had it written into the message, the calling thread would
    // later fetch every track's points from the other core's cache, which cost as much as the thread saved.)
    void computeDepths(const Tracklets& ts, const float* cloud, size_t n_pts) {
        const size_t n = ts.tracks.size();
        const bool from_sweep = seq_.fromSweep(ts, cloud, n_pts);
        if (from_sweep && prefetch_open_ && prefetch_stamp_ == ts.stamps.front() && prefetch_n_ == n) {  // started by prefetchDepth
            prefetch_open_ = false;
            seq_.depth.assign(n, -1.f);
            checkCall(ctx_, limo_depth_estimate_end(ctx_, seq_.depth.data(), n), "limo_depth_estimate_end");
            ++seq_.stats.depth_prefetched;
        } else if (from_sweep) {
            closeOpenDepthCall();
            seq_.stageFeatures(ts);
            const Camera& cam = *seq_.camera;
            checkCall(ctx_,
                      limo_depth_estimate(ctx_, cloud, n_pts, T_cam_lidar_.data(), cam.focal_length, cam.principal_point[0], cam.principal_point[1], p_.image_width,
                                          p_.image_height, seq_.uv.data(), n, seq_.ground.data(), &depth_params_, seq_.depth.data()),
                      "limo_depth_estimate");
        }
        seq_.recordDepths(ts, from_sweep);
    }

    StreamParams p_;
    Pose T_cam_lidar_;
    stream_detail::Sequence seq_;  // (after p_: it refers to it)
    limo_ctx* ctx_ = nullptr;      // of the depth calls
    limo_ctx* five_point_ctx_ = nullptr;  // of estimateFivePoint, made at its first call
    limo_depth_params depth_params_;
    bool prefetch_open_ = false;  // prefetchDepth: a limo_depth_estimate_begin whose frame process() has not seen yet
    TimestampNSec prefetch_stamp_ = 0;
    size_t prefetch_n_ = 0;
    std::thread worker_;  // the depth thread and its one job slot
    std::mutex job_mutex_;
    std::condition_variable job_cv_;
    JobState job_state_ = JobState::Idle;
    const Tracklets* job_ts_ = nullptr;
    bool job_has_stamp_ = false;  // identity of the job's frame, read from the message when the job starts
    TimestampNSec job_stamp_ = 0;
    size_t job_tracks_ = 0;
    const float* job_cloud_ = nullptr;
    size_t job_n_pts_ = 0;
    std::exception_ptr job_error_;
    bool ahead_valid_ = false;  // the sequence's point_d holds the depths the depth thread computed for the message (ahead_stamp_, ahead_tracks_)
    TimestampNSec ahead_stamp_ = 0;
    size_t ahead_tracks_ = 0;
    const Tracklets* next_tracklets_ = nullptr;  // announceNextFrame
    const float* next_cloud_ = nullptr;
    size_t next_n_pts_ = 0;
};

}  // namespace keyframe_bundle_adjustment
