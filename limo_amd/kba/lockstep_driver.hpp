// lockstep_driver.hpp — N sequences of one sensor rig driven in lock step: the phases of a frame (stream_detail::Sequence, sequence.hpp)
// that StreamDriver (stream_driver.hpp) runs for one sequence, with ONE device call per stage and tick for all the sequences that want it:
//   frames of the tick
//     -> limo_depth_estimate_batch                    the sweeps of the tick (feature staging, depth history: per sequence, host)
//     -> motion prior                                 external, constant velocity (host), or the five-point prior: matches and gate
//                                                     per sequence, the estimates through one limo_five_point_batch
//                                                     (StreamParams::five_point_on_device; off: the host estimator per sequence)
//     -> limo_ba_adjust_pose_only_batch[_each]        every frame without an external prior (_each: the jobs' options differ)
//     -> keyframe selection (host, per sequence), then the pushes of all sequences: one limo_landmark_init over the concatenated rays
//     -> for the sequences whose solve is due: window cut + labels (host), limo_landmark_select_batch
//        (StreamParams::landmark_selection_on_device; off: the host selector per sequence), limo_ba_batch_create / _solve[_each] /
//        _download
//     -> pose of the frame, motion, statistics
// A sequence without a frame in a tick sits out; sequences may start late, end early and solve on different ticks.  Every sequence is
// a stream_detail::Sequence of its own: the policy of a frame is that type's, this file holds the calls.  What the batched entry points
// promise (include/limo_hip.h: "window / frame / pool i gets the bytes of its single call") makes the pose rows of sequence i those of
// a StreamDriver given the same frames, byte for byte.
// Threads: the phases run on `host_threads` threads, one sequence on one thread at a time (no phase touches a limo_ctx); only the
// thread that calls tick() calls the C-ABI, on the driver's one context.  No result depends on host_threads.
// Where the library behind the C-ABI lacks a batched entry point, that stage loops over the single call.  Stats counts both.
// Not here: the depth assignment one frame ahead (there is no begin / end form of the batch call), the iteration table
// (BundleAdjusterKeyframes::minimizer_progress_to_stdout_), different rigs per sequence, per-sequence parameters of the depth,
// five-point and selection batches or of the solve schedule (the outlier-rejection thresholds and quantiles, the shrubbery weight
// and the keyframe / window policy MAY differ per sequence: the second constructor), several GPUs.
#pragma once
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>

#include "sequence.hpp"

namespace keyframe_bundle_adjustment {

namespace lockstep_detail {

// run(n, fn): fn(k) for k = 0 .. n-1 on the pool's threads and the calling one; returns when all are done.  Every k runs even when
// one throws; the exception of the smallest k is rethrown (so which one is reported does not depend on the number of threads).
class HostPool {
public:
    explicit HostPool(int threads) {
        for (int i = 1; i < threads; ++i) workers_.emplace_back([this] { workerMain(); });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            exit_ = true;
        }
        wake_.notify_all();
        for (auto& w : workers_) w.join();
    }
    HostPool(const HostPool&) = delete;
    HostPool& operator=(const HostPool&) = delete;

    void run(size_t n, const std::function<void(size_t)>& fn) {
        std::vector<std::exception_ptr> errors(n);
        const std::function<void(size_t)> body = [&](size_t k) {
            try {
                fn(k);
            } catch (...) {
                errors[k] = std::current_exception();
            }
        };
        if (workers_.empty() || n < 2) {
            for (size_t k = 0; k < n; ++k) body(k);
        } else {
            {
                std::lock_guard<std::mutex> lk(m_);
                job_ = &body;
                n_ = n;
                next_ = 0;
                pending_ = n;
            }
            wake_.notify_all();
            work();
            std::unique_lock<std::mutex> lk(m_);
            done_.wait(lk, [this] { return pending_ == 0; });
            job_ = nullptr;
        }
        for (const auto& e : errors)
            if (e) std::rethrow_exception(e);
    }

private:
    void work() {
        for (;;) {
            size_t k;
            const std::function<void(size_t)>* job;
            {
                std::lock_guard<std::mutex> lk(m_);
                if (!job_ || next_ >= n_) return;
                k = next_++;
                job = job_;
            }
            (*job)(k);  // (run() does not return, and `body` lives, while an item is pending)
            {
                std::lock_guard<std::mutex> lk(m_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    void workerMain() {
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
            wake_.wait(lk, [this] { return exit_ || (job_ && next_ < n_); });
            if (exit_) return;
            lk.unlock();
            work();
            lk.lock();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable wake_, done_;
    const std::function<void(size_t)>* job_ = nullptr;
    size_t n_ = 0, next_ = 0, pending_ = 0;
    bool exit_ = false;
};

}  // namespace lockstep_detail

// The batched entry points are weak references, as limo_five_point is in stream_driver.hpp: where the library behind the C-ABI lacks one
// (the test backends tests/cpp/emu_pipeline.cpp and oracle_abi.cpp) its address is null and tick() loops over the single call.
#pragma weak limo_depth_estimate_batch
#pragma weak limo_five_point
#pragma weak limo_five_point_default_params
#pragma weak limo_five_point_batch
#pragma weak limo_ba_adjust_pose_only_batch
#pragma weak limo_ba_adjust_pose_only_batch_each
#pragma weak limo_ctx_set_pose_covariance
#pragma weak limo_ctx_last_pose_covariance
#pragma weak limo_ba_batch_solve_each
#pragma weak limo_landmark_select
#pragma weak limo_landmark_select_batch
#pragma weak limo_ba_batch_create
#pragma weak limo_ba_batch_solve
#pragma weak limo_ba_batch_download
#pragma weak limo_ba_batch_destroy

class LockstepDriver {
public:
    using Sequence = stream_detail::Sequence;
    struct Rig {  // what the batched depth and selection calls take ONE of: every sequence must bring the same
        Camera::Ptr camera;
        EigenPose T_camera_lidar;
    };
    struct Frame {  // what StreamDriver::process is given: the tracker's message (handed over), the sweep, a prior if the caller has one
        Tracklets tracklets;
        const float* cloud_xyzi = nullptr;
        size_t n_pts = 0;
        bool has_external_prior = false;
        EigenPose external_prior;
    };
    // One stage of the tick.  batched_calls: calls of the batched entry point, items: what they carried (frames, windows, pushes, pools),
    // max_items: the most one call carried; fallback_calls: single calls made because the library lacks the batched entry point or
    // refused the batch.  per_window_calls (pose_only, solve): batched calls whose jobs carried DIFFERING options - the _each entry
    // points (a backend without them gets one batched call per group of equal options instead, and counts none here).
    // sec_host: the per-sequence host phase in front of the call (on the pool), sec_abi: inside the C-ABI.
    struct Stage {
        long batched_calls = 0, items = 0, fallback_calls = 0, per_window_calls = 0;
        int max_items = 0;
        double sec_host = 0., sec_abi = 0.;
    };
    struct Stats {
        int ticks = 0, frames = 0;
        Stage depth, five_point, pose_only, landmark_init, select, solve;
        long landmarks_initialised = 0;    // landmarks the landmark_init calls carried
        long five_point_host = 0;          // five-point estimates of the host estimator (flag off, or no device entry point at all)
        long select_host = 0;              // selections of the host selector (flag off, no entry point, or a pool the device refuses)
        double sec_host_finish = 0.;       // commit of the solves + book-keeping
        double sec_total = 0.;
    };

    // host_threads <= 0: min(N, 16) (never the machine's core count: a GPU node shares its cores)
    // (all sequences with the same parameters)
    LockstepDriver(const StreamParams& p, const std::vector<Rig>& rigs, int host_threads = 0)
            : LockstepDriver(std::vector<StreamParams>(std::max<size_t>(rigs.size(), 1), p), rigs, host_threads) {}
    // One StreamParams per sequence - a sweep over outlier-rejection parameters side by side (the reference's tune_parameters_kitti.py).
    // May differ: robust_loss_depth_thres, robust_loss_reprojection_thres, outlier_rejection_quantile, shrubbery_weight,
    // max_size_optimization_window, min_number_connecting_landmarks, min_median_flow, critical_rotation_difference,
    // time_between_keyframes_sec, height_over_ground, prior_speed - host phases of the sequence, or options that travel with its
    // window.  Every other field must be equal: outlier_rejection_num_iterations and solver_time_sec decide the schedule of a batched
    // solve, the rest parameterises a batched depth, five-point or selection call (max_size_optimization_window among them while the
    // device selection is on: it sizes that call's add rules).  A difference there is refused, the way a differing rig is.
    LockstepDriver(const std::vector<StreamParams>& ps, const std::vector<Rig>& rigs, int host_threads = 0)
            : ps_(ps), p_(ps_.empty() ? fallback_params_ : ps_[0]),
              host_threads_(host_threads > 0 ? host_threads : (int)std::min<size_t>(std::max<size_t>(rigs.size(), 1), 16)), pool_(host_threads_) {
        if (rigs.empty()) throw std::invalid_argument("LockstepDriver: no sequence");
        if (ps_.size() != rigs.size()) throw std::invalid_argument("LockstepDriver: " + std::to_string(ps_.size()) + " parameter sets for " + std::to_string(rigs.size()) + " sequences");
        for (size_t i = 1; i < ps_.size(); ++i)
            if (const char* field = fixedDifference(ps_[0], ps_[i]))
                throw std::invalid_argument("LockstepDriver: the parameters of sequence " + std::to_string(i) + " differ from sequence 0's in " + field +
                                            ": it decides the schedule of a batched solve or parameterises a batched depth, five-point or selection call, which take one "
                                            "value; drive it with a StreamDriver of its own");
        for (size_t i = 0; i < rigs.size(); ++i) {
            if (!rigs[i].camera) throw std::invalid_argument("LockstepDriver: sequence " + std::to_string(i) + " has no camera");
            if (!sameRig(rigs[0], rigs[i]))
                throw std::invalid_argument("LockstepDriver: the rig of sequence " + std::to_string(i) +
                                            " differs from sequence 0's (camera intrinsics, camera <- vehicle or camera <- lidar): the batched depth and selection "
                                            "calls take one rig; drive it with a StreamDriver of its own");
        }
        const bool five_point_device = p_.five_point_on_device && &limo_five_point_default_params != nullptr && (&limo_five_point_batch != nullptr || &limo_five_point != nullptr);
        for (size_t i = 0; i < rigs.size(); ++i) seqs_.push_back(std::make_unique<Sequence>(ps_[i], rigs[i].camera, five_point_device, (int)i));
        T_cam_lidar_ = convert(rigs[0].T_camera_lidar);
        ctx_ = createContext();
        limo_depth_default_params(&depth_params_);
    }
    ~LockstepDriver() {
        if (ctx_) limo_ctx_destroy(ctx_);
    }
    LockstepDriver(const LockstepDriver&) = delete;
    LockstepDriver& operator=(const LockstepDriver&) = delete;

    size_t size() const { return seqs_.size(); }
    int hostThreads() const { return host_threads_; }

    // One tick: frames[i] is sequence i's frame, or empty (the sequence sits out).  The tracklets are taken over (depths are filled in).
    // Six stages, each: a phase of stream_detail::Sequence over the sequences of the tick (on the pool), the jobs of those that want the
    // stage's call gathered, the ONE batched call (or, without the entry point, the single calls), the results back into the jobs.
    void tick(std::vector<std::optional<Frame>>& frames) {
        using stream_detail::Timed;
        if (frames.size() != seqs_.size()) throw std::invalid_argument("LockstepDriver::tick: one (optional) frame per sequence");
        const auto t_begin = std::chrono::steady_clock::now();
        std::vector<Sequence*> act;
        for (size_t i = 0; i < seqs_.size(); ++i) {
            if (!frames[i] || frames[i]->tracklets.stamps.empty()) continue;  // (an empty message: :98-104)
            Frame& f = *frames[i];
            seqs_[i]->take(std::move(f.tracklets), f.cloud_xyzi, f.n_pts, f.has_external_prior ? &f.external_prior : nullptr);
            frames[i].reset();
            act.push_back(seqs_[i].get());
        }
        ++stats_.ticks;
        if (act.empty()) return;
        const Camera& cam = *seqs_[0]->camera;  // (one rig)
        const double f = cam.focal_length, cx = cam.principal_point[0], cy = cam.principal_point[1];

        // ---- 1. depth: one call over the sweeps of the tick
        host(act, stats_.depth.sec_host, [](Sequence& s, size_t) { s.stageDepth(); });
        {
            const auto sweep = those(act, &Sequence::wantsSweep);
            Timed t(stats_.depth.sec_abi);
            if (sweep.empty()) {
            } else if (&limo_depth_estimate_batch != nullptr) {
                std::vector<limo_depth_frame> fr;
                for (Sequence* s : sweep) fr.push_back(s->depthFrame(s->tracklets, s->cloud, s->n_pts));
                check(limo_depth_estimate_batch(ctx_, (int32_t)fr.size(), fr.data(), T_cam_lidar_.data(), f, cx, cy, p_.image_width, p_.image_height, &depth_params_, 0u),
                      "limo_depth_estimate_batch");
                batched(stats_.depth, sweep.size());
            } else {
                for (Sequence* s : sweep) {
                    const limo_depth_frame fr = s->depthFrame(s->tracklets, s->cloud, s->n_pts);
                    check(limo_depth_estimate(ctx_, fr.cloud_xyzi, fr.n_pts, T_cam_lidar_.data(), f, cx, cy, p_.image_width, p_.image_height, fr.feat_uv, fr.n_feat,
                                              fr.feat_is_ground, &depth_params_, fr.depth_out),
                          "limo_depth_estimate");
                    ++stats_.depth.fallback_calls;
                }
            }
        }

        // ---- 2. depth history and prior; the five-point estimates through one call
        host(act, stats_.five_point.sec_host, [](Sequence& s, size_t) {
            s.recordDepth();
            s.applyDepths();
            s.choosePrior();
        });
        {
            const auto est = those(act, &Sequence::wantsFivePoint);
            for (const Sequence* s : act) stats_.five_point_host += s->estimatedOnHost();
            Timed t(stats_.five_point.sec_abi);
            if (!est.empty()) {
                limo_five_point_params prm;
                limo_five_point_default_params(&prm);
                std::vector<limo_five_point_frame> fr;
                for (Sequence* s : est) fr.push_back(s->fivePointFrame());
                std::vector<limo_five_point_motion> mo(est.size());
                if (&limo_five_point_batch != nullptr) {
                    check(limo_five_point_batch(ctx_, (int32_t)fr.size(), fr.data(), f, cx, cy, &prm, mo.data()), "limo_five_point_batch");
                    batched(stats_.five_point, est.size());
                } else {
                    for (size_t k = 0; k < est.size(); ++k) {
                        check(limo_five_point(ctx_, &fr[k], f, cx, cy, &prm, &mo[k], nullptr), "limo_five_point");
                        ++stats_.five_point.fallback_calls;
                    }
                }
                for (size_t k = 0; k < est.size(); ++k) est[k]->acceptFivePoint(mo[k]);
            }
        }

        // ---- 3. Keyframe(prior) per sequence, one pose-only call for every frame that wants one
        host(act, stats_.pose_only.sec_host, [](Sequence& s, size_t) { s.buildKeyframe(); });
        {
            const auto ref = those(act, &Sequence::wantsPoseOnly);
            Timed t(stats_.pose_only.sec_abi);
            // pose covariance (StreamParams::pose_covariance): the call ends with the library's pass when a sequence of it asks, and
            // window `window` of the call that has just returned goes into the job of the sequence it belongs to
            bool want_cov = false;
            for (Sequence* s : ref) want_cov = want_cov || s->p.pose_covariance;
            want_cov = want_cov && &limo_ctx_set_pose_covariance != nullptr && &limo_ctx_last_pose_covariance != nullptr;
            if (!ref.empty() && &limo_ctx_set_pose_covariance != nullptr) check(limo_ctx_set_pose_covariance(ctx_, want_cov ? 1 : 0), "limo_ctx_set_pose_covariance");
            auto fetch_cov = [&](Sequence* s, size_t window) {
                if (!want_cov || !s->p.pose_covariance) return;
                BundleAdjusterKeyframes::WindowJob& j = s->pose_job;
                j.cov.assign((size_t)36 * j.window->n_kf * j.window->n_kf, 0.);
                check(limo_ctx_last_pose_covariance(ctx_, (int32_t)window, (int64_t)j.cov.size(), j.cov.data(), &j.cov_status), "limo_ctx_last_pose_covariance");
            };
            if (ref.empty()) {
            } else if (&limo_ba_adjust_pose_only_batch != nullptr) {
                std::vector<limo_ba_window> ws;
                std::vector<limo_speed_prior> priors;
                for (Sequence* s : ref) {
                    ws.push_back(*s->pose_job.window);
                    priors.push_back(s->pose_job.prior);  // (speed_weight 0: "no prior for this window")
                }
                std::vector<limo_ba_report> reports(ref.size());
                // the jobs' own options: all equal - today's call; else one call with an entry per window, or (a backend without it)
                // one call per group of equal options.  No window is ever solved with another window's options.
                std::vector<limo_ba_options> opts;
                for (Sequence* s : ref) opts.push_back(s->pose_job.opts);
                const std::vector<std::vector<size_t>> groups = optionGroups(opts);
                if (groups.size() == 1) {
                    check(limo_ba_adjust_pose_only_batch(ctx_, (int32_t)ws.size(), ws.data(), priors.data(), &opts[0], reports.data()), "limo_ba_adjust_pose_only_batch");
                    batched(stats_.pose_only, ref.size());
                    for (size_t k = 0; k < ref.size(); ++k) fetch_cov(ref[k], k);
                } else if (&limo_ba_adjust_pose_only_batch_each != nullptr) {
                    check(limo_ba_adjust_pose_only_batch_each(ctx_, (int32_t)ws.size(), ws.data(), priors.data(), opts.data(), reports.data()), "limo_ba_adjust_pose_only_batch_each");
                    batched(stats_.pose_only, ref.size());
                    ++stats_.pose_only.per_window_calls;
                    for (size_t k = 0; k < ref.size(); ++k) fetch_cov(ref[k], k);
                } else {
                    for (const std::vector<size_t>& g : groups) {
                        std::vector<limo_ba_window> gw;
                        std::vector<limo_speed_prior> gp;
                        for (size_t k : g) gw.push_back(ws[k]), gp.push_back(priors[k]);
                        std::vector<limo_ba_report> gr(g.size());
                        check(limo_ba_adjust_pose_only_batch(ctx_, (int32_t)gw.size(), gw.data(), gp.data(), &opts[g[0]], gr.data()), "limo_ba_adjust_pose_only_batch");
                        for (size_t i = 0; i < g.size(); ++i) reports[g[i]] = gr[i];
                        for (size_t i = 0; i < g.size(); ++i) fetch_cov(ref[g[i]], i);
                        batched(stats_.pose_only, g.size());
                    }
                }
                for (size_t k = 0; k < ref.size(); ++k) ref[k]->pose_job.report = reports[k];
            } else {
                for (Sequence* s : ref) {
                    BundleAdjusterKeyframes::WindowJob& j = s->pose_job;
                    check(limo_ba_adjust_pose_only(ctx_, j.window, j.has_prior ? &j.prior : nullptr, &j.opts, &j.report), "limo_ba_adjust_pose_only");
                    fetch_cov(s, 0);
                    ++stats_.pose_only.fallback_calls;
                }
            }
            if (want_cov) check(limo_ctx_set_pose_covariance(ctx_, 0), "limo_ctx_set_pose_covariance");  // (the tick's solves do not pay for the pass)
        }

        // ---- 4. keyframe selection per sequence, the pushes of all sequences through one limo_landmark_init
        host(act, stats_.landmark_init.sec_host, [](Sequence& s, size_t) { s.selectKeyframe(); });
        {
            const auto pushes = those(act, &Sequence::wantsPush);
            size_t n_lm = 0, n_rays = 0;
            for (Sequence* s : pushes) {
                n_lm += s->push.ids.size();
                n_rays += s->push.rays.size();
            }
            Timed t(stats_.landmark_init.sec_abi);
            if (n_lm > 0) {  // (a push that introduces no landmark makes no call in the single driver either)
                std::vector<int32_t> off{0};
                std::vector<limo_ray> rays;
                std::vector<uint8_t> use_depth, ok(n_lm, 0);
                std::vector<double> pos(3 * n_lm, 0.0);
                off.reserve(n_lm + 1), rays.reserve(n_rays), use_depth.reserve(n_lm);
                for (Sequence* s : pushes) {
                    const BundleAdjusterKeyframes::PushJob& j = s->push;
                    const int32_t base = (int32_t)rays.size();
                    for (size_t l = 0; l < j.ids.size(); ++l) off.push_back(base + j.off[l + 1]);
                    rays.insert(rays.end(), j.rays.begin(), j.rays.end());
                    use_depth.insert(use_depth.end(), j.use_depth.begin(), j.use_depth.end());
                }
                check(limo_landmark_init(ctx_, (int32_t)n_lm, off.data(), rays.data(), use_depth.data(), pos.data(), ok.data()), "limo_landmark_init");
                size_t at = 0;
                for (Sequence* s : pushes) {
                    BundleAdjusterKeyframes::PushJob& j = s->push;
                    std::copy(pos.begin() + 3 * at, pos.begin() + 3 * (at + j.ids.size()), j.pos.begin());
                    std::copy(ok.begin() + at, ok.begin() + at + j.ids.size(), j.ok.begin());
                    at += j.ids.size();
                }
                batched(stats_.landmark_init, pushes.size());
                stats_.landmarks_initialised += (long)n_lm;
            }
        }

        // ---- 5. window stage of the sequences whose solve is due: cut + labels, selection, solve
        host(act, stats_.select.sec_host, [](Sequence& s, size_t) { s.enterWindow(); });
        const auto due = those(act, &Sequence::wantsSolve), pools = those(act, &Sequence::wantsSelection);
        stats_.select_host += (long)(due.size() - pools.size());
        if (!pools.empty()) {
            std::vector<uint8_t> ok(pools.size(), 0);
            {
                Timed t(stats_.select.sec_abi);
                if (&limo_landmark_select_batch != nullptr) {
                    std::vector<limo_select_pool> ps;
                    std::vector<uint8_t*> outs;
                    for (Sequence* s : pools) {
                        ps.push_back(s->select.pool);
                        outs.push_back(s->select.out.data());
                    }
                    // (every sequence's parameters say the same: one StreamParams)
                    if (limo_landmark_select_batch(ctx_, (int32_t)ps.size(), ps.data(), pools[0]->select.params, outs.data()) == LIMO_OK) {
                        batched(stats_.select, pools.size());
                        ok.assign(pools.size(), 1);
                    }
                }
                if (!ok[0])  // no batched entry point, or a pool the device does not take (above 64 keyframes or 8 cameras): pool by pool
                    for (size_t k = 0; k < pools.size(); ++k) {
                        ok[k] = limo_landmark_select(ctx_, &pools[k]->select.pool, pools[k]->select.params, pools[k]->select.out.data()) == LIMO_OK;
                        ++stats_.select.fallback_calls;
                        stats_.select_host += !ok[k];
                    }
            }
            host(pools, stats_.solve.sec_host, [&](Sequence& s, size_t k) { s.selectionDone(ok[k] != 0); });
        }
        if (!due.empty()) {
            Timed t(stats_.solve.sec_abi);
            if (&limo_ba_batch_create != nullptr && &limo_ba_batch_solve != nullptr && &limo_ba_batch_download != nullptr && &limo_ba_batch_destroy != nullptr) {
                // one resident batch over `which` of the due sequences: create, solve (each: an entry of options per window), download
                auto solveBatch = [&](const std::vector<size_t>& which, const std::vector<limo_ba_options>& opts, bool each) {
                    std::vector<limo_ba_window> ws;
                    for (size_t k : which) ws.push_back(*due[k]->solve_job.window);
                    std::vector<limo_ba_report> reports(which.size());
                    limo_ba_batch* b = nullptr;
                    check(limo_ba_batch_create(ctx_, (int32_t)ws.size(), ws.data(), &b), "limo_ba_batch_create");
                    int rc = each ? limo_ba_batch_solve_each(b, (int32_t)opts.size(), opts.data()) : limo_ba_batch_solve(b, &opts[0]);
                    const char* what = each ? "limo_ba_batch_solve_each" : "limo_ba_batch_solve";
                    if (rc == LIMO_OK) {
                        rc = limo_ba_batch_download(b, ws.data(), reports.data());
                        what = "limo_ba_batch_download";
                    }
                    const std::string err = rc != LIMO_OK ? limo_last_error(ctx_) : "";
                    limo_ba_batch_destroy(b);
                    if (rc != LIMO_OK) throw std::runtime_error(std::string(what) + ": " + err);
                    for (size_t i = 0; i < which.size(); ++i) due[which[i]]->solve_job.report = reports[i];
                    batched(stats_.solve, which.size());
                };
                // (the jobs' own options: as in the pose-only stage)
                std::vector<limo_ba_options> opts;
                std::vector<size_t> all;
                for (size_t k = 0; k < due.size(); ++k) opts.push_back(due[k]->solve_job.opts), all.push_back(k);
                const std::vector<std::vector<size_t>> groups = optionGroups(opts);
                if (groups.size() == 1) {
                    solveBatch(all, opts, false);
                } else if (&limo_ba_batch_solve_each != nullptr) {
                    solveBatch(all, opts, true);
                    ++stats_.solve.per_window_calls;
                } else {
                    for (const std::vector<size_t>& g : groups) solveBatch(g, {opts[g[0]]}, false);
                }
            } else {
                for (Sequence* s : due) {
                    BundleAdjusterKeyframes::WindowJob& j = s->solve_job;
                    check(limo_ba_solve(ctx_, j.window, &j.opts, &j.report), "limo_ba_solve");
                    ++stats_.solve.fallback_calls;
                }
            }
        }

        // ---- 6. the solved windows back, pose of the frame, motion, statistics
        host(act, stats_.sec_host_finish, [](Sequence& s, size_t) { s.finishFrame(); });
        stats_.frames += (int)act.size();
        stats_.sec_total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    }

    // KITTI odometry rows of sequence i: those of a StreamDriver given the same frames
    void writeKittiTrajectory(size_t i, std::ostream& os) const { seqs_.at(i)->writeKittiTrajectory(os); }
    void writeCovariances(size_t i, std::ostream& os) const { seqs_.at(i)->writeCovariances(os); }  // (StreamParams::pose_covariance)

    BundleAdjusterKeyframes& adjuster(size_t i) { return seqs_.at(i)->ba; }
    const std::vector<EigenPose>& poses(size_t i) const { return seqs_.at(i)->poses; }
    // (the counts; its seconds are the host phases' own statements - the calls are this driver's, per stage)
    const StreamStats& sequenceStats(size_t i) const { return seqs_.at(i)->stats; }
    const std::string& lastSummary(size_t i) const { return seqs_.at(i)->last_summary; }
    const Stats& stats() const { return stats_; }
    limo_depth_params& depthParams() { return depth_params_; }

private:
    static bool sameRig(const Rig& a, const Rig& b) {
        if (!a.camera || !b.camera) return false;
        bool same = a.camera->focal_length == b.camera->focal_length && a.camera->principal_point[0] == b.camera->principal_point[0] &&
                    a.camera->principal_point[1] == b.camera->principal_point[1];
        for (int i = 0; i < 7; ++i) same = same && a.camera->pose_camera_vehicle[i] == b.camera->pose_camera_vehicle[i];
        for (int i = 0; i < 9; ++i) same = same && a.T_camera_lidar.R[i] == b.T_camera_lidar.R[i];
        for (int i = 0; i < 3; ++i) same = same && a.T_camera_lidar.t[i] == b.T_camera_lidar.t[i];
        return same;
    }
    // The first field of b that must equal a's and does not (see the second constructor), or null.
    static const char* fixedDifference(const StreamParams& a, const StreamParams& b) {
#define KBA_LOCKSTEP_FIXED(f) \
    if (!(a.f == b.f)) return #f;
        KBA_LOCKSTEP_FIXED(outlier_rejection_num_iterations)
        KBA_LOCKSTEP_FIXED(solver_time_sec)
        KBA_LOCKSTEP_FIXED(motion_prior)
        KBA_LOCKSTEP_FIXED(five_point_on_device)
        KBA_LOCKSTEP_FIXED(landmark_selection_on_device)
        KBA_LOCKSTEP_FIXED(max_number_landmarks_near_bin)
        KBA_LOCKSTEP_FIXED(max_number_landmarks_middle_bin)
        KBA_LOCKSTEP_FIXED(max_number_landmarks_far_bin)
        KBA_LOCKSTEP_FIXED(roi_middle)
        KBA_LOCKSTEP_FIXED(roi_far)
        KBA_LOCKSTEP_FIXED(voxel_size_xyz)
        KBA_LOCKSTEP_FIXED(add_ground_landmarks_per_keyframe)
        KBA_LOCKSTEP_FIXED(add_depth_landmarks_newest)
        KBA_LOCKSTEP_FIXED(assign_depth)
        KBA_LOCKSTEP_FIXED(depth_ahead)
        KBA_LOCKSTEP_FIXED(image_width)
        KBA_LOCKSTEP_FIXED(image_height)
        KBA_LOCKSTEP_FIXED(ground_labels)
#undef KBA_LOCKSTEP_FIXED
        if (a.landmark_selection_on_device && a.add_ground_landmarks_per_keyframe > 0 && a.max_size_optimization_window != b.max_size_optimization_window)
            return "max_size_optimization_window (with landmark_selection_on_device it sizes the selection call's add rules)";
        return nullptr;
    }
    static bool sameOptions(const limo_ba_options& a, const limo_ba_options& b) {
        return a.depth_thres == b.depth_thres && a.reprojection_thres == b.reprojection_thres && a.depth_quantile == b.depth_quantile &&
               a.reprojection_quantile == b.reprojection_quantile && a.num_trim_rounds == b.num_trim_rounds && a.trim_solver_iterations == b.trim_solver_iterations &&
               a.min_landmarks_for_trimming == b.min_landmarks_for_trimming && a.minimum_number_residual_groups == b.minimum_number_residual_groups &&
               a.max_num_iterations == b.max_num_iterations && a.max_solver_time_sec == b.max_solver_time_sec && a.function_tolerance == b.function_tolerance &&
               a.gradient_tolerance == b.gradient_tolerance && a.parameter_tolerance == b.parameter_tolerance &&
               a.initial_trust_region_radius == b.initial_trust_region_radius && a.max_trust_region_radius == b.max_trust_region_radius &&
               a.min_trust_region_radius == b.min_trust_region_radius && a.min_lm_diagonal == b.min_lm_diagonal && a.max_lm_diagonal == b.max_lm_diagonal &&
               a.min_relative_decrease == b.min_relative_decrease && a.max_num_consecutive_invalid_steps == b.max_num_consecutive_invalid_steps &&
               a.jacobi_scaling == b.jacobi_scaling;
    }
    // the jobs of a call by equal options: groups of indices, each in job order, the groups in the order of their first job
    static std::vector<std::vector<size_t>> optionGroups(const std::vector<limo_ba_options>& opts) {
        std::vector<std::vector<size_t>> groups;
        for (size_t k = 0; k < opts.size(); ++k) {
            size_t g = 0;
            while (g < groups.size() && !sameOptions(opts[groups[g][0]], opts[k])) ++g;
            if (g == groups.size()) groups.emplace_back();
            groups[g].push_back(k);
        }
        return groups;
    }
    // a phase over `which` on the pool: fn(sequence, its index in `which`)
    template <class Phase>
    void host(const std::vector<Sequence*>& which, double& sec, Phase fn) {
        stream_detail::Timed t(sec);
        pool_.run(which.size(), [&](size_t k) { fn(*which[k], k); });
    }
    // the sequences whose last phase left a job for the stage's call
    static std::vector<Sequence*> those(const std::vector<Sequence*>& act, bool (Sequence::*wants)() const) {
        std::vector<Sequence*> out;
        for (Sequence* s : act)
            if ((s->*wants)()) out.push_back(s);
        return out;
    }
    void check(int rc, const char* what) const { checkCall(ctx_, rc, what); }
    static void batched(Stage& st, size_t items) {
        ++st.batched_calls;
        st.items += (long)items;
        st.max_items = std::max(st.max_items, (int)items);
    }

    std::vector<StreamParams> ps_;   // one per sequence (fixed at construction: the sequences refer to their entry)
    const StreamParams fallback_params_{};
    const StreamParams& p_;          // ps_[0]: what the batched depth, five-point and selection calls take (equal in every entry)
    int host_threads_ = 1;
    lockstep_detail::HostPool pool_;  // (after host_threads_: built from it)
    std::vector<std::unique_ptr<Sequence>> seqs_;  // (after ps_: they refer to it)
    Pose T_cam_lidar_;
    limo_ctx* ctx_ = nullptr;
    limo_depth_params depth_params_;
    Stats stats_;
};

}  // namespace keyframe_bundle_adjustment
