// lockstep_driver.hpp — N sequences of one sensor rig driven in lock step: the stages of StreamDriver::process (stream_driver.hpp), in
// the same order, with ONE device call per stage and tick for all the sequences that need it:
//   frames of the tick
//     -> limo_depth_estimate_batch                    the sweeps of the tick (feature staging, depth history: per sequence, host)
//     -> motion prior                                 external, constant velocity (host), or the five-point prior: matches and gate
//                                                     per sequence, the estimates through one limo_five_point_batch
//                                                     (StreamParams::five_point_on_device; off: the host estimator per sequence)
//     -> limo_ba_adjust_pose_only_batch               every frame without an external prior
//     -> keyframe selection (host, per sequence), then the pushes of all sequences: one limo_landmark_init over the concatenated rays
//     -> for the sequences whose solve is due: window cut + labels (host), limo_landmark_select_batch
//        (StreamParams::landmark_selection_on_device; off: the host selector per sequence), limo_ba_batch_create / _solve / _download
//     -> pose of the frame, motion, statistics
// A sequence without a frame in a tick sits out; sequences may start late, end early and solve on different ticks.  Every sequence
// keeps its own adjuster, keyframe selector, depth history, motion state, statistics and pose list; the per-sequence pieces of a frame
// are stream_detail's (stream_driver.hpp), the halves around each device call BundleAdjusterKeyframes' prepare / commit.  What the
// batched entry points promise (include/limo_hip.h: "window / frame / pool i gets the bytes of its single call") makes the pose rows of
// sequence i those of a StreamDriver given the same frames, byte for byte.
// Threads: the per-sequence host phases (Keyframe object, prepare, commit, host selection) run on `host_threads` threads, one sequence
// on one thread at a time; only the thread that calls tick() calls the C-ABI, on the driver's one context.  No result depends on
// host_threads.
// The batched symbols are weak references, as limo_five_point is in stream_driver.hpp: where the library behind the C-ABI lacks one
// (the test backends tests/cpp/emu_pipeline.cpp and oracle_abi.cpp) that stage loops over the single call.  Stats counts both.
// Not here: the depth assignment one frame ahead (there is no begin / end form of the batch call), the iteration table
// (BundleAdjusterKeyframes::minimizer_progress_to_stdout_), different rigs or parameters per sequence, several GPUs.
#pragma once
#include <functional>
#include <optional>

#include "stream_driver.hpp"

#pragma weak limo_depth_estimate_batch
#pragma weak limo_five_point_batch
#pragma weak limo_ba_adjust_pose_only_batch
#pragma weak limo_landmark_select
#pragma weak limo_landmark_select_batch
#pragma weak limo_ba_batch_create
#pragma weak limo_ba_batch_solve
#pragma weak limo_ba_batch_download
#pragma weak limo_ba_batch_destroy

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

class LockstepDriver {
public:
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
    // refused the batch.  sec_host: the per-sequence host phase in front of the call (on the pool), sec_abi: inside the C-ABI.
    struct Stage {
        long batched_calls = 0, items = 0, fallback_calls = 0;
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
    LockstepDriver(const StreamParams& p, const std::vector<Rig>& rigs, int host_threads = 0)
            : p_(p), host_threads_(host_threads > 0 ? host_threads : (int)std::min<size_t>(std::max<size_t>(rigs.size(), 1), 16)), pool_(host_threads_) {
        if (rigs.empty()) throw std::invalid_argument("LockstepDriver: no sequence");
        for (size_t i = 0; i < rigs.size(); ++i) {
            if (!rigs[i].camera) throw std::invalid_argument("LockstepDriver: sequence " + std::to_string(i) + " has no camera");
            if (!sameRig(rigs[0], rigs[i]))
                throw std::invalid_argument("LockstepDriver: the rig of sequence " + std::to_string(i) +
                                            " differs from sequence 0's (camera intrinsics, camera <- vehicle or camera <- lidar): the batched depth and selection "
                                            "calls take one rig; drive it with a StreamDriver of its own");
        }
        for (size_t i = 0; i < rigs.size(); ++i) {
            seqs_.push_back(std::make_unique<Seq>());
            Seq& s = *seqs_.back();
            s.camera = rigs[i].camera;
            s.ba.dump_tag_ = (int)i;
            stream_detail::configureSequence(p, s.ba, s.selector);
        }
        T_cam_lidar_ = convert(rigs[0].T_camera_lidar);
        int dev = 0;  // LIMO_DEVICE: the GPU of this driver
        if (const char* e = std::getenv("LIMO_DEVICE")) dev = std::atoi(e);
        if (limo_ctx_create(dev, &ctx_) != LIMO_OK) throw std::runtime_error("LockstepDriver: no HIP device (limo_ctx_create)");
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
    void tick(std::vector<std::optional<Frame>>& frames) {
        using clk = std::chrono::steady_clock;
        auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
        if (frames.size() != seqs_.size()) throw std::invalid_argument("LockstepDriver::tick: one (optional) frame per sequence");
        const auto t_begin = clk::now();
        std::vector<Seq*> act;
        for (size_t i = 0; i < seqs_.size(); ++i) {
            Seq& s = *seqs_[i];
            if (!frames[i] || frames[i]->tracklets.stamps.empty()) continue;  // (an empty message: :98-104)
            s.tracklets = std::move(frames[i]->tracklets);
            s.cloud = frames[i]->cloud_xyzi;
            s.n_pts = frames[i]->n_pts;
            s.has_external = frames[i]->has_external_prior;
            s.external = frames[i]->external_prior;
            frames[i].reset();
            act.push_back(&s);
        }
        ++stats_.ticks;
        if (act.empty()) return;
        auto host = [&](std::vector<Seq*>& which, double& sec, const std::function<void(Seq&)>& fn) {
            const auto t0 = clk::now();
            pool_.run(which.size(), [&](size_t k) { fn(*which[k]); });
            sec += since(t0);
        };

        // ---- 1. depth: staging per sequence, one call over the sweeps of the tick, history per sequence
        host(act, stats_.depth.sec_host, [&](Seq& s) {
            s.stamp = s.tracklets.stamps.front();
            s.want_five_point = s.want_pose_only = s.want_push = s.want_solve = false;
            s.is_keyframe = false;
            const size_t n = s.tracklets.tracks.size();
            s.from_sweep = p_.assign_depth && s.cloud && s.n_pts && n;
            if (s.from_sweep) {
                s.depth.assign(n, -1.f);
                stream_detail::stageFeatures(p_, s.tracklets, s.uv, s.ground);
            }
        });
        {
            std::vector<Seq*> sweep;
            for (Seq* s : act)
                if (s->from_sweep) sweep.push_back(s);
            const auto t0 = clk::now();
            const Camera& cam = *seqs_[0]->camera;
            if (sweep.empty()) {
            } else if (&limo_depth_estimate_batch != nullptr) {
                std::vector<limo_depth_frame> fr;
                for (Seq* s : sweep) fr.push_back({s->cloud, s->n_pts, s->uv.data(), s->tracklets.tracks.size(), s->ground.data(), s->depth.data()});
                check(limo_depth_estimate_batch(ctx_, (int32_t)fr.size(), fr.data(), T_cam_lidar_.data(), cam.focal_length, cam.principal_point[0], cam.principal_point[1],
                                                p_.image_width, p_.image_height, &depth_params_, 0u),
                      "limo_depth_estimate_batch");
                batched(stats_.depth, sweep.size());
            } else {
                for (Seq* s : sweep) {
                    check(limo_depth_estimate(ctx_, s->cloud, s->n_pts, T_cam_lidar_.data(), cam.focal_length, cam.principal_point[0], cam.principal_point[1], p_.image_width,
                                              p_.image_height, s->uv.data(), s->tracklets.tracks.size(), s->ground.data(), &depth_params_, s->depth.data()),
                          "limo_depth_estimate");
                    ++stats_.depth.fallback_calls;
                }
            }
            stats_.depth.sec_abi += since(t0);
        }

        // ---- 2. prior.  The first frame of a sequence is a Pose-fixed keyframe at the origin (:305-326): its push is prepared here.
        const bool five_point_prior = p_.motion_prior == StreamParams::MotionPrior::FivePoint;
        const bool five_point_device = p_.five_point_on_device && &limo_five_point_default_params != nullptr && (&limo_five_point_batch != nullptr || &limo_five_point != nullptr);
        host(act, stats_.five_point.sec_host, [&](Seq& s) {
            if (s.history.counts(s.tracklets)) s.stats.features += (int)s.tracklets.tracks.size();
            s.history.record(s.tracklets, s.from_sweep ? s.depth.data() : nullptr, s.point_d, s.stats.features_with_depth);
            s.history.forgetEndedTracks(s.tracklets);
            stream_detail::applyDepths(s.tracklets, s.point_d);
            s.first = s.ba.keyframes_.empty();
            s.pose = EigenPose::Identity();
            Plane ground_plane;
            ground_plane.distance = p_.height_over_ground;
            if (s.first) {
                Keyframe first(s.stamp, s.tracklets, s.camera, EigenPose::Identity(), Keyframe::FixationStatus::Pose, ground_plane);
                first.freezeMeasurements();  // (this driver owns its keyframes and never edits their measurements_: the table may outlive the call)
                s.ba.preparePush(std::move(first), s.push);
                s.want_push = s.is_keyframe = true;
            } else if (s.has_external) {
                s.prior = s.external;
            } else if (five_point_prior) {
                s.stamp_last_kf = s.ba.getKeyframe().timestamp_;
                stream_detail::fivePointQuery(s.tracklets, s.stamp_last_kf, s.stamp, s.five_point_query);
                if (s.five_point_query.estimate) {
                    ++s.stats.five_point_calls;
                    if (five_point_device)
                        s.want_five_point = true;
                    else
                        s.last_five_point = stream_detail::fivePointOnHost(s.five_point_query, *s.camera, (uint64_t)s.stamp);
                }
            } else {
                s.prior = s.motion.constantVelocityPrior(p_, s.stamp);
            }
        });
        {
            std::vector<Seq*> est;
            for (Seq* s : act) {
                if (s->want_five_point) est.push_back(s);
                stats_.five_point_host += !s->first && !s->has_external && five_point_prior && s->five_point_query.estimate && !s->want_five_point;
            }
            const auto t0 = clk::now();
            if (!est.empty()) {
                const Camera& cam = *seqs_[0]->camera;
                limo_five_point_params prm;
                limo_five_point_default_params(&prm);
                std::vector<limo_five_point_frame> fr;
                for (Seq* s : est) fr.push_back(stream_detail::fivePointFrame(s->five_point_query, (uint64_t)s->stamp));
                std::vector<limo_five_point_motion> mo(est.size());
                if (&limo_five_point_batch != nullptr) {
                    check(limo_five_point_batch(ctx_, (int32_t)fr.size(), fr.data(), cam.focal_length, cam.principal_point[0], cam.principal_point[1], &prm, mo.data()),
                          "limo_five_point_batch");
                    batched(stats_.five_point, est.size());
                } else {
                    for (size_t k = 0; k < est.size(); ++k) {
                        check(limo_five_point(ctx_, &fr[k], cam.focal_length, cam.principal_point[0], cam.principal_point[1], &prm, &mo[k], nullptr), "limo_five_point");
                        ++stats_.five_point.fallback_calls;
                    }
                }
                for (size_t k = 0; k < est.size(); ++k) {
                    est[k]->last_five_point = stream_detail::fivePointMotion(mo[k]);
                    ++est[k]->stats.five_point_device_calls;
                }
            }
            stats_.five_point.sec_abi += since(t0);
        }

        // ---- 3. Keyframe(prior) per sequence, one pose-only call for every frame without an external prior (:192-211)
        std::vector<Seq*> later;  // the sequences past their first frame
        for (Seq* s : act)
            if (!s->first) later.push_back(s);
        host(later, stats_.pose_only.sec_host, [&](Seq& s) {
            if (!s.has_external && five_point_prior) {
                const EigenPose motion = stream_detail::fivePointUnscaled(p_, *s.camera, s.five_point_query, s.five_point_query.estimate ? &s.last_five_point : nullptr,
                                                                          s.stamp_last_kf, s.stamp);
                s.prior = stream_detail::fivePointPrior(s.ba, s.stamp, motion);
            }
            s.prior = stream_detail::normalisedPrior(s.prior);
            Plane ground_plane;
            ground_plane.distance = p_.height_over_ground;
            s.cur = std::make_shared<Keyframe>(s.stamp, s.tracklets, s.camera, s.prior, Keyframe::FixationStatus::None, ground_plane);
            s.cur->freezeMeasurements();  // (as above: built once per keyframe, kept for its life in the window)
            if (!s.has_external) {  // a prior without scale is always refined against the fixed landmarks of the last selection
                s.ba.preparePoseOnly(*s.cur, s.pose_job);
                s.want_pose_only = true;
            }
        });
        {
            std::vector<Seq*> ref;
            for (Seq* s : later)
                if (s->want_pose_only) ref.push_back(s);
            const auto t0 = clk::now();
            if (ref.empty()) {
            } else if (&limo_ba_adjust_pose_only_batch != nullptr) {
                std::vector<limo_ba_window> ws;
                std::vector<limo_speed_prior> priors;
                for (Seq* s : ref) {
                    ws.push_back(*s->pose_job.window);
                    priors.push_back(s->pose_job.prior);  // (speed_weight 0: "no prior for this window")
                }
                std::vector<limo_ba_report> reports(ref.size());
                check(limo_ba_adjust_pose_only_batch(ctx_, (int32_t)ws.size(), ws.data(), priors.data(), &ref[0]->pose_job.opts, reports.data()), "limo_ba_adjust_pose_only_batch");
                for (size_t k = 0; k < ref.size(); ++k) ref[k]->pose_job.report = reports[k];
                batched(stats_.pose_only, ref.size());
            } else {
                for (Seq* s : ref) {
                    BundleAdjusterKeyframes::WindowJob& j = s->pose_job;
                    check(limo_ba_adjust_pose_only(ctx_, j.window, j.has_prior ? &j.prior : nullptr, &j.opts, &j.report), "limo_ba_adjust_pose_only");
                    ++stats_.pose_only.fallback_calls;
                }
            }
            stats_.pose_only.sec_abi += since(t0);
        }

        // ---- 4. keyframe selection per sequence (:218-222), the pushes of all sequences through one limo_landmark_init (:231-233)
        host(later, stats_.landmark_init.sec_host, [&](Seq& s) {
            if (s.want_pose_only) {
                s.ba.commitPoseOnly(s.pose_job);
                stream_detail::trace(s.ba, "pose-only", s.stamp, s.cur->pose_, s.ba.last_report_.final_cost);
            }
            s.pose = s.cur->getEigenPose();
            const auto selected = s.selector.select({s.cur}, s.ba.getActiveKeyframePtrs());
            if (!selected.empty()) {
                if (selected.size() != 1 || *selected.begin() != s.cur) throw std::logic_error("LockstepDriver: the keyframe selector returned a frame it was not given");
                s.ba.preparePush(std::move(*s.cur), s.push);  // (this frame's keyframe object is not looked at again: handed over)
                s.want_push = s.is_keyframe = true;
            }
        });
        {
            std::vector<Seq*> pushes;
            size_t n_lm = 0, n_rays = 0;
            for (Seq* s : act)
                if (s->want_push) {
                    pushes.push_back(s);
                    n_lm += s->push.ids.size();
                    n_rays += s->push.rays.size();
                }
            const auto t0 = clk::now();
            if (n_lm > 0) {  // (a push that introduces no landmark makes no call in the single driver either)
                std::vector<int32_t> off{0};
                std::vector<limo_ray> rays;
                std::vector<uint8_t> use_depth, ok(n_lm, 0);
                std::vector<double> pos(3 * n_lm, 0.0);
                off.reserve(n_lm + 1), rays.reserve(n_rays), use_depth.reserve(n_lm);
                for (Seq* s : pushes) {
                    const BundleAdjusterKeyframes::PushJob& j = s->push;
                    const int32_t base = (int32_t)rays.size();
                    for (size_t l = 0; l < j.ids.size(); ++l) off.push_back(base + j.off[l + 1]);
                    rays.insert(rays.end(), j.rays.begin(), j.rays.end());
                    use_depth.insert(use_depth.end(), j.use_depth.begin(), j.use_depth.end());
                }
                check(limo_landmark_init(ctx_, (int32_t)n_lm, off.data(), rays.data(), use_depth.data(), pos.data(), ok.data()), "limo_landmark_init");
                size_t at = 0;
                for (Seq* s : pushes) {
                    BundleAdjusterKeyframes::PushJob& j = s->push;
                    std::copy(pos.begin() + 3 * at, pos.begin() + 3 * (at + j.ids.size()), j.pos.begin());
                    std::copy(ok.begin() + at, ok.begin() + at + j.ids.size(), j.ok.begin());
                    at += j.ids.size();
                }
                batched(stats_.landmark_init, pushes.size());
                stats_.landmarks_initialised += (long)n_lm;
            }
            stats_.landmark_init.sec_abi += since(t0);
        }

        // ---- 5. window stage of the sequences whose solve is due (:245-263): cut + labels, selection, solve
        host(act, stats_.select.sec_host, [&](Seq& s) {
            if (s.want_push) s.ba.commitPush(s.push);
            s.push.kf.reset();
            if (s.first) return;
            s.now_sec = convert(s.stamp);
            if (!stream_detail::solveDue(p_, s.ba, s.now_sec, s.last_solved_sec)) return;
            s.ba.deactivateKeyframes(p_.min_number_connecting_landmarks, 3, p_.max_size_optimization_window);
            s.ba.updateLabels(s.tracklets, p_.shrubbery_weight);
            s.ba.prepareSelection(s.select);
            s.want_solve = true;
            if (!s.select.on_device) {  // the host selector: no call to wait for
                s.ba.commitSelection(s.select, false);
                s.ba.prepareSolve(s.solve_job);
            }
        });
        std::vector<Seq*> due, pools;
        for (Seq* s : act)
            if (s->want_solve) {
                due.push_back(s);
                if (s->select.on_device)
                    pools.push_back(s);
                else
                    ++stats_.select_host;
            }
        if (!pools.empty()) {
            const auto t0 = clk::now();
            bool done = false;
            if (&limo_landmark_select_batch != nullptr) {
                std::vector<limo_select_pool> ps;
                std::vector<uint8_t*> outs;
                for (Seq* s : pools) {
                    ps.push_back(s->select.pool);
                    outs.push_back(s->select.out.data());
                }
                // (every sequence's parameters say the same: one StreamParams)
                done = limo_landmark_select_batch(ctx_, (int32_t)ps.size(), ps.data(), pools[0]->select.params, outs.data()) == LIMO_OK;
                if (done) batched(stats_.select, pools.size());
                for (Seq* s : pools) s->select_ok = done;
            }
            if (!done)  // no batched entry point, or a pool the device does not take (above 64 keyframes or 8 cameras): pool by pool
                for (Seq* s : pools) {
                    s->select_ok = limo_landmark_select(ctx_, &s->select.pool, s->select.params, s->select.out.data()) == LIMO_OK;
                    ++stats_.select.fallback_calls;
                    stats_.select_host += !s->select_ok;
                }
            stats_.select.sec_abi += since(t0);
            host(pools, stats_.solve.sec_host, [&](Seq& s) {
                s.ba.commitSelection(s.select, s.select_ok);
                s.ba.prepareSolve(s.solve_job);
            });
        }
        if (!due.empty()) {
            const auto t0 = clk::now();
            if (&limo_ba_batch_create != nullptr && &limo_ba_batch_solve != nullptr && &limo_ba_batch_download != nullptr && &limo_ba_batch_destroy != nullptr) {
                std::vector<limo_ba_window> ws;
                for (Seq* s : due) ws.push_back(*s->solve_job.window);
                std::vector<limo_ba_report> reports(due.size());
                limo_ba_batch* b = nullptr;
                check(limo_ba_batch_create(ctx_, (int32_t)ws.size(), ws.data(), &b), "limo_ba_batch_create");
                int rc = limo_ba_batch_solve(b, &due[0]->solve_job.opts);
                const char* what = "limo_ba_batch_solve";
                if (rc == LIMO_OK) {
                    rc = limo_ba_batch_download(b, ws.data(), reports.data());
                    what = "limo_ba_batch_download";
                }
                const std::string err = rc != LIMO_OK ? limo_last_error(ctx_) : "";
                limo_ba_batch_destroy(b);
                if (rc != LIMO_OK) throw std::runtime_error(std::string(what) + ": " + err);
                for (size_t k = 0; k < due.size(); ++k) due[k]->solve_job.report = reports[k];
                batched(stats_.solve, due.size());
            } else {
                for (Seq* s : due) {
                    BundleAdjusterKeyframes::WindowJob& j = s->solve_job;
                    check(limo_ba_solve(ctx_, j.window, &j.opts, &j.report), "limo_ba_solve");
                    ++stats_.solve.fallback_calls;
                }
            }
            stats_.solve.sec_abi += since(t0);
        }

        // ---- 6. book-keeping: the optimised pose if the frame became a keyframe, its prior otherwise (:281-294)
        host(act, stats_.sec_host_finish, [&](Seq& s) {
            if (s.want_solve) {
                s.last_summary = s.ba.commitSolve(s.solve_job);
                ++s.stats.solves;
                stream_detail::trace(s.ba, "solve", s.stamp, s.ba.getKeyframe().pose_, s.ba.last_report_.final_cost);
                s.stats.solves_on_non_keyframes += !s.is_keyframe;
                s.last_solved_sec = s.now_sec;
            }
            if (!s.first && s.ba.getKeyframe().timestamp_ == s.stamp) s.pose = s.ba.getKeyframe().getEigenPose();
            s.motion.advance(s.pose, s.stamp);
            ++s.stats.frames;
            s.stats.keyframes += s.is_keyframe;
            s.poses.push_back(s.pose);
            s.cur.reset();
            s.pose_job.flat.reset(), s.solve_job.flat.reset(), s.select.flat.reset();
        });
        stats_.frames += (int)act.size();
        stats_.sec_total += since(t_begin);
    }

    // KITTI odometry rows of sequence i (StreamDriver::writeKittiTrajectory)
    void writeKittiTrajectory(size_t i, std::ostream& os) const {
        const Seq& s = *seqs_.at(i);
        const EigenPose cv = s.camera->getEigenPose();
        for (const auto& pose_kf_origin : s.poses) {
            const EigenPose m = cv * pose_kf_origin.inverse() * cv.inverse();
            char buf[512];
            std::snprintf(buf, sizeof(buf), "%.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g", m.R[0], m.R[1], m.R[2], m.t[0], m.R[3], m.R[4],
                          m.R[5], m.t[1], m.R[6], m.R[7], m.R[8], m.t[2]);
            os << buf << "\n";
        }
    }

    BundleAdjusterKeyframes& adjuster(size_t i) { return seqs_.at(i)->ba; }
    const std::vector<EigenPose>& poses(size_t i) const { return seqs_.at(i)->poses; }
    const StreamDriver::Stats& sequenceStats(size_t i) const { return seqs_.at(i)->stats; }  // (the counts; the seconds are the driver's, per stage)
    const std::string& lastSummary(size_t i) const { return seqs_.at(i)->last_summary; }
    const Stats& stats() const { return stats_; }
    limo_depth_params& depthParams() { return depth_params_; }

private:
    struct Seq {
        Camera::Ptr camera;
        BundleAdjusterKeyframes ba;
        KeyframeSelector selector;
        stream_detail::DepthHistory history;
        stream_detail::MotionState motion;
        StreamDriver::Stats stats;
        std::vector<EigenPose> poses;
        double last_solved_sec = -1e30;
        std::string last_summary;
        five_point::Motion last_five_point;
        std::vector<float> uv, depth, point_d;
        std::vector<uint8_t> ground;
        // the frame of this tick
        Tracklets tracklets;
        const float* cloud = nullptr;
        size_t n_pts = 0;
        bool has_external = false, from_sweep = false, first = false, is_keyframe = false;
        bool want_five_point = false, want_pose_only = false, want_push = false, want_solve = false, select_ok = false;
        EigenPose external, prior, pose;
        TimestampNSec stamp = 0, stamp_last_kf = 0;
        double now_sec = 0.;
        Keyframe::Ptr cur;
        stream_detail::FivePointQuery five_point_query;
        BundleAdjusterKeyframes::PushJob push;
        BundleAdjusterKeyframes::WindowJob pose_job, solve_job;
        BundleAdjusterKeyframes::SelectJob select;
    };

    static bool sameRig(const Rig& a, const Rig& b) {
        if (!a.camera || !b.camera) return false;
        bool same = a.camera->focal_length == b.camera->focal_length && a.camera->principal_point[0] == b.camera->principal_point[0] &&
                    a.camera->principal_point[1] == b.camera->principal_point[1];
        for (int i = 0; i < 7; ++i) same = same && a.camera->pose_camera_vehicle[i] == b.camera->pose_camera_vehicle[i];
        for (int i = 0; i < 9; ++i) same = same && a.T_camera_lidar.R[i] == b.T_camera_lidar.R[i];
        for (int i = 0; i < 3; ++i) same = same && a.T_camera_lidar.t[i] == b.T_camera_lidar.t[i];
        return same;
    }
    void check(int rc, const char* what) const {
        if (rc != LIMO_OK) throw std::runtime_error(std::string(what) + ": " + limo_last_error(ctx_));
    }
    static void batched(Stage& st, size_t items) {
        ++st.batched_calls;
        st.items += (long)items;
        st.max_items = std::max(st.max_items, (int)items);
    }

    StreamParams p_;
    int host_threads_ = 1;
    lockstep_detail::HostPool pool_;  // (after host_threads_: built from it)
    std::vector<std::unique_ptr<Seq>> seqs_;
    Pose T_cam_lidar_;
    limo_ctx* ctx_ = nullptr;
    limo_depth_params depth_params_;
    Stats stats_;
};

}  // namespace keyframe_bundle_adjustment
