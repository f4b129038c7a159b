// limo_stream — ROS-free streaming visual odometry on a synthetic KITTI-00-shaped drive (BASELINE.json configs[4]):
//   per frame: 64-beam sweep + tracked features -> StreamDriver (limo_depth_estimate -> adjustPoseOnly -> keyframe
//   selection -> push -> deactivateKeyframes -> solve) -> KITTI pose row.
// The replacement of the reference's demo application (demo_keyframe_bundle_adjustment_meta/apps/main_program/
// main_program.cpp:39-216 reads KITTI data from disk and plays it through the ROS nodes; there is no dataset here, so the
// drive is synthesised by synth_world.hpp) and of the node's callback (limo_amd/kba/stream_driver.hpp).
//
//   limo_stream [--frames N] [--features N] [--az N] [--seed S] [--window K] [--poses out.txt] [--gt-poses gt.txt]
//               [--dump-velodyne DIR] [--velodyne DIR] [--no-depth] [--depth-ahead thread|stream|none] [--quiet]
//               [--depth-params FILE] [--progress] [--covariance FILE] [--five-point-prior [--five-point-host | --five-point-device]]
//               [--select-host | --select-device] [--depth-thres A] [--reprojection-thres A] [--outlier-quantile Q] [--shrubbery-weight W]
//               [--sequences N [--frames-step K] [--stagger S] [--host-threads T] [--sweep FILE]]
// --depth-thres / --reprojection-thres / --outlier-quantile / --shrubbery-weight set the outlier rejection of solve() and adjustPoseOnly()
// (the node's robust_loss_depth_thres, robust_loss_reprojection_thres, outlier_rejection_quantile, shrubbery_weight) for a single drive
// and for every sequence of a lock-step one.  --sweep FILE (with --sequences N) gives sequence i the parameters of line i of FILE:
// key=value tokens with the keys depth_thres, reprojection_thres, outlier_quantile, shrubbery_weight, window; a missing key takes the
// command line's value.  Every sequence of a sweep drives the SAME world - seed --seed for all, not seed + i - so the per-sequence part of
// the JSON line, which echoes each sequence's parameters next to its ATE, is the sweep's result (the reference's
// tune_parameters_kitti.py, side by side on one GPU).
// --sequences N drives N sequences in lock step through ONE LockstepDriver (limo_amd/kba/lockstep_driver.hpp: one batched device call
// per stage and tick for all of them) instead of one StreamDriver: sequence i is the synthetic drive of --seed (seed + i), runs
// frames - i*K frames (--frames-step K) and gets its first frame at tick i*S (--stagger S); --host-threads T sets the threads of the
// per-sequence host phases (default min(N, 16)).  --poses P writes P.0 .. P.(N-1), each the bytes the single drive of that seed and frame
// count writes; the last line printed is one JSON object: sequences, aggregate frames_per_s, per stage the batched calls, what they
// carried and the single-call fallbacks, per-sequence ATE.  No --progress, --velodyne, --dump-velodyne in this form; --depth-ahead is ignored (a tick assigns its own depths).
// --five-point-prior takes the frame's motion prior from the five-point algorithm, as the reference's node does without a tf prior
// (mono_lidar.cpp:157-186), instead of constant velocity; --five-point-host / --five-point-device say where its RANSAC runs (the host
// estimator five_point.hpp, or limo_five_point) instead of StreamParams' default.  Same pose rows, bit for bit.
// --select-host / --select-device say where solve() selects its landmarks (the host selector, or limo_landmark_select) instead of
// StreamParams' default.  Same pose rows, bit for bit.
// --covariance FILE writes one row per frame: the 36 numbers (row-major 6 x 6: rotation 3 | translation 3, the tangent units of
// include/limo_hip.h, "Pose covariance") of the marginal covariance of the frame's adjustPoseOnly and its limo_cov_status; a frame that
// was not refined (the first one) has zeros and LIMO_COV_NOT_COMPUTED, a frame before the first solve() - no landmark selected yet, nothing
// constrains its pose - NaN and LIMO_COV_RANK_DEFICIENT.  With --sequences N: FILE.i per sequence.  No pose row changes.
// --progress prints Ceres' per-iteration table for every adjustPoseOnly and solve to stdout, as the reference's node does
// (BundleAdjusterKeyframes::minimizer_progress_to_stdout_); the pose rows do not change.
// --depth-params reads the depth estimator's settings from a mono_lidar_fusion_parameters.yaml (the file the reference
// application loads; limo_amd/kba/depth_params_yaml.hpp) instead of using the built-in defaults, which are that file's values.
// --dump-velodyne writes every synthetic sweep as a KITTI velodyne scan (DIR/NNNNNN.bin); --velodyne replays scans from
// such a directory instead of ray-casting them (the scans of a real KITTI sequence have the same format; the tracked
// features of a real sequence come from the feature tracker, which is outside this path).
// The sweeps are received into page-locked buffers (limo_host_alloc) and the input runs one frame ahead of the pipeline: the driver
// assigns the depths of frame t+1 while the pose refinement and the solve of frame t run (StreamDriver::announceNextFrame) - the
// reference's depth estimator is a process of its own beside the BA node.  --depth-ahead thread (default): a thread of the driver does
// it; stream: the calling thread starts it on the driver's own HIP stream and collects it at the next frame (limo_depth_estimate_begin
// / _end); none (= --no-prefetch): every frame's depths are assigned inside its own process() call.  Same pose rows, bit for bit.
// Prints one summary line per run and `key value` lines for scripts: fps of the pipeline (input synthesis excluded and
// reported separately), ATE against the ground truth, share of features that received a LiDAR depth.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <optional>
#include <sstream>
#include <string>

#include "../../limo_amd/kba/depth_params_yaml.hpp"
#include "../../limo_amd/kba/kitti_io.hpp"
#include "../../limo_amd/kba/lockstep_driver.hpp"
#include "../../limo_amd/kba/stream_driver.hpp"
#include "synth_world.hpp"

using namespace keyframe_bundle_adjustment;

namespace {

// a frame as the sensor drivers deliver it: the tracker's message and the sweep in a page-locked buffer
struct Frame {
    Tracklets ts;
    float* scan = nullptr;
    size_t cap = 0, n_pts = 0, n_tracks = 0;
};

// the sensors of one synthetic drive: frame t's sweep and the tracker's message for it (frames are asked for in order)
struct Synth {
    Synth(synth_world::World& w, uint64_t seed, int n_feat_, const std::string& replay, const std::string& dump)
            : world(w), rng(seed * 31 + 1), n_feat(n_feat_), replay_dir(replay), dump_dir(dump) {}
    synth_world::World& world;
    std::mt19937_64 rng;
    int n_feat;
    std::string replay_dir, dump_dir;
    const int history = 10;
    std::vector<int> live;  // landmarks tracked in the previous frame
    std::map<int, int> first_seen;
    std::vector<float> cloud;
    std::vector<uint8_t> cloud_ground;
    size_t n_points = 0;

    bool frame(int t, Frame& out) {
        world.sweep(t, cloud, cloud_ground);  // (also labels the returns that hit the ground: the features' class labels come from it)
        if (!replay_dir.empty()) {
            std::vector<float> scan;
            if (!kitti_io::readVelodyneBin(kitti_io::velodynePath(replay_dir, t), scan) || scan.size() != cloud.size()) {
                std::fprintf(stderr, "limo_stream: cannot replay %s\n", kitti_io::velodynePath(replay_dir, t).c_str());
                return false;
            }
            cloud.swap(scan);
        }
        if (!dump_dir.empty() && !kitti_io::writeVelodyneBin(kitti_io::velodynePath(dump_dir, t), cloud.data(), cloud.size() / 4)) {
            std::fprintf(stderr, "limo_stream: cannot write %s\n", kitti_io::velodynePath(dump_dir, t).c_str());
            return false;
        }
        n_points += cloud.size() / 4;
        if (cloud.size() > out.cap) {
            if (out.scan) limo_host_free(out.scan);
            out.cap = cloud.size() + cloud.size() / 8;
            out.scan = static_cast<float*>(limo_host_alloc(out.cap * sizeof(float)));
            if (!out.scan) {
                std::fprintf(stderr, "limo_stream: limo_host_alloc failed\n");
                return false;
            }
        }
        std::memcpy(out.scan, cloud.data(), cloud.size() * sizeof(float));
        out.n_pts = cloud.size() / 4;
        // tracks that survive into this frame (still visible, not occluded), then new ones up to n_feat
        const Vector3d here = world.origin_veh[t].translation();
        const std::vector<int> near = world.boxes_near(here, 70.);
        std::vector<int> now;
        for (int id : live) {
            double u, v, z;
            if (world.visible(t, world.lms[id], near, u, v, z)) now.push_back(id);
        }
        if ((int)now.size() < n_feat) {
            const size_t before = world.lms.size();
            world.spawn(t, cloud, cloud_ground, n_feat - (int)now.size(), rng);
            for (size_t id = before; id < world.lms.size(); ++id) {
                now.push_back((int)id);
                first_seen[(int)id] = t;
            }
        }
        Tracklets ts;
        for (int k = 0; k < history && t - k >= 0; ++k) ts.stamps.push_back((uint64_t)(t - k) * 50000000ull + 1000ull);
        for (int id : now) {
            Tracklet tr;
            tr.id = id;
            const int age = std::min(history, t - first_seen[id] + 1);
            for (int k = 0; k < age; ++k) {
                double u, v, z;
                if (!world.project(t - k, world.lms[id].p, u, v, z)) break;
                double n3[3];
                synth_world::hash_normals((uint64_t)(t - k) * 1000003ull + (uint64_t)id, n3);
                tr.feature_points.push_back(FeaturePoint((float)(u + 0.3 * n3[0]), (float)(v + 0.3 * n3[1])));  // d < 0: the driver fills it
            }
            if (tr.feature_points.empty()) continue;
            tr.age = tr.feature_points.size();
            tr.label = world.lms[id].ground ? 7 : 11;  // cityscapes road / building
            ts.tracks.push_back(tr);
        }
        live = now;
        out.n_tracks = ts.tracks.size();
        out.ts = std::move(ts);
        return true;
    }
};

// --sequences N: N synthetic drives (seed, seed + 1, ...) through one LockstepDriver.  Sequence i runs frames - i * frames_step frames and
// gets its first frame at tick i * stagger; every tick hands the driver the frames that are due.  The input of a tick is synthesised
// before the tick and timed apart from it, as in the single drive.
struct LockstepOptions {
    int sequences = 0, frames_step = 0, stagger = 0, host_threads = 0, perturb_rig = -1, perturb_trim_rounds = -1;
    int n_frames = 200, n_feat = 1500, n_az = 2000;
    uint64_t seed = 7;
    std::string poses_path, gt_path, depth_params_path, sweep_path, covariance_path;
    bool quiet = false;
};

// --sweep FILE: line i gives sequence i's parameters as key=value tokens - depth_thres, reprojection_thres, outlier_quantile,
// shrubbery_weight, window; a key a line does not set keeps the command line's value (`base`).  false: err says why.
bool read_sweep(const std::string& path, int n, const StreamParams& base, std::vector<StreamParams>& out, std::string& err) {
    std::ifstream f(path);
    if (!f) {
        err = "cannot read " + path;
        return false;
    }
    out.clear();
    std::string line;
    while (std::getline(f, line)) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        StreamParams p = base;
        std::istringstream tokens(line);
        std::string tok;
        while (tokens >> tok) {
            const size_t eq = tok.find('=');
            const std::string key = tok.substr(0, eq), val = eq == std::string::npos ? "" : tok.substr(eq + 1);
            char* end = nullptr;
            const double v = std::strtod(val.c_str(), &end);
            if (val.empty() || *end) {
                err = "line " + std::to_string(out.size() + 1) + ": `" + tok + "` is not key=number";
                return false;
            }
            if (key == "depth_thres") p.robust_loss_depth_thres = v;
            else if (key == "reprojection_thres") p.robust_loss_reprojection_thres = v;
            else if (key == "outlier_quantile") p.outlier_rejection_quantile = v;
            else if (key == "shrubbery_weight") p.shrubbery_weight = v;
            else if (key == "window") p.max_size_optimization_window = (int)v;
            else {
                err = "line " + std::to_string(out.size() + 1) + ": unknown key `" + key + "` (depth_thres, reprojection_thres, outlier_quantile, shrubbery_weight, window)";
                return false;
            }
        }
        out.push_back(p);
    }
    if ((int)out.size() != n) {
        err = std::to_string(out.size()) + " lines for " + std::to_string(n) + " sequences";
        return false;
    }
    return true;
}

int run_lockstep(const LockstepOptions& o, StreamParams sp) {
    using clk = std::chrono::steady_clock;
    const int N = o.sequences;
    const bool sweep = !o.sweep_path.empty();  // every sequence drives the SAME world (the seed), with a parameter set of its own
    struct Drive {
        std::unique_ptr<synth_world::World> world;
        std::unique_ptr<Synth> synth;
        Camera::Ptr cam;
        Frame frame;
        int n_frames = 0, first_tick = 0;
        uint64_t seed = 0;
    };
    std::vector<Drive> drives(N);
    std::vector<LockstepDriver::Rig> rigs;
    int n_ticks = 0, total_frames = 0;
    for (int i = 0; i < N; ++i) {
        Drive& d = drives[i];
        d.n_frames = o.n_frames - i * o.frames_step;
        d.first_tick = i * o.stagger;
        if (d.n_frames <= 0) {
            std::fprintf(stderr, "limo_stream: --frames-step leaves sequence %d without a frame\n", i);
            return 2;
        }
        d.seed = sweep ? o.seed : o.seed + (uint64_t)i;
        d.world = std::make_unique<synth_world::World>(d.n_frames, d.seed);
        d.world->n_az = o.n_az;
        d.synth = std::make_unique<Synth>(*d.world, d.seed, o.n_feat, std::string(), std::string());
        // --perturb-rig I (testing aid): sequence I comes with another focal length - the driver must refuse it
        d.cam = std::make_shared<Camera>(d.world->f + (i == o.perturb_rig ? 1. : 0.), Vector2d(d.world->cx, d.world->cy), d.world->cam_veh);
        rigs.push_back({d.cam, d.world->cam_lidar});
        n_ticks = std::max(n_ticks, d.first_tick + d.n_frames);
        total_frames += d.n_frames;
    }
    sp.image_width = (int)drives[0].world->W;
    sp.image_height = (int)drives[0].world->H;
    std::vector<StreamParams> sps(N, sp);
    if (sweep) {
        std::string err;
        if (!read_sweep(o.sweep_path, N, sp, sps, err)) {
            std::fprintf(stderr, "limo_stream: --sweep: %s\n", err.c_str());
            return 2;
        }
    }
    // --perturb-trim-rounds I (testing aid): sequence I comes with another number of trimming rounds - the driver must refuse it
    if (o.perturb_trim_rounds >= 0 && o.perturb_trim_rounds < N) sps[o.perturb_trim_rounds].outlier_rejection_num_iterations += 1;
    std::unique_ptr<LockstepDriver> driver;
    try {
        driver = std::make_unique<LockstepDriver>(sps, rigs, o.host_threads);
    } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "limo_stream: %s\n", e.what());
        return 2;
    }
    if (!o.depth_params_path.empty()) {
        std::string err;
        if (!depth_params_yaml::load(o.depth_params_path, &driver->depthParams(), &err)) {
            std::fprintf(stderr, "limo_stream: --depth-params %s\n", err.c_str());
            return 2;
        }
    }
    auto release = [&]() {
        for (Drive& d : drives)
            if (d.frame.scan) limo_host_free(d.frame.scan);
    };
    double sec_synth = 0., sec_pipeline = 0.;
    std::vector<std::optional<LockstepDriver::Frame>> tick(N);
    for (int T = 0; T < n_ticks; ++T) {
        const auto t0 = clk::now();
        for (int i = 0; i < N; ++i) {
            Drive& d = drives[i];
            const int t = T - d.first_tick;
            tick[i].reset();
            if (t < 0 || t >= d.n_frames) continue;
            if (!d.synth->frame(t, d.frame)) {
                release();
                return 1;
            }
            tick[i].emplace();
            tick[i]->tracklets = std::move(d.frame.ts);  // (the tracker's message is handed over: the driver fills in depths)
            tick[i]->cloud_xyzi = d.frame.scan;
            tick[i]->n_pts = d.frame.n_pts;
        }
        const auto t1 = clk::now();
        driver->tick(tick);
        const auto t2 = clk::now();
        sec_synth += std::chrono::duration<double>(t1 - t0).count();
        sec_pipeline += std::chrono::duration<double>(t2 - t1).count();
        if (!o.quiet && (T % 100 == 0 || T == n_ticks - 1)) {
            std::printf("tick %d: %d frames so far\n", T, driver->stats().frames);
            std::fflush(stdout);
        }
    }
    release();
    const LockstepDriver::Stats& st = driver->stats();
    std::string per_sequence;
    for (int i = 0; i < N; ++i) {
        const Drive& d = drives[i];
        const auto& poses = driver->poses(i);
        double se = 0., worst = 0.;
        for (int t = 0; t < d.n_frames; ++t) {
            const Vector3d e = poses[t].inverse().translation() - d.world->origin_veh[t].translation();
            se += e.norm() * e.norm();
            worst = std::max(worst, e.norm());
        }
        const double ate = std::sqrt(se / d.n_frames);
        if (!o.poses_path.empty()) {
            std::ofstream f(o.poses_path + "." + std::to_string(i));
            driver->writeKittiTrajectory(i, f);
        }
        if (!o.covariance_path.empty()) {
            std::ofstream f(o.covariance_path + "." + std::to_string(i));
            driver->writeCovariances(i, f);
        }
        if (!o.gt_path.empty()) {
            std::ofstream f(o.gt_path + "." + std::to_string(i));
            const EigenPose cv = d.cam->getEigenPose();
            for (int t = 0; t < d.n_frames; ++t) kitti_io::writePoseRow(f, kitti_io::inCameraFrame(cv, d.world->origin_veh[t]));
        }
        const StreamDriver::Stats& ss = driver->sequenceStats(i);
        std::printf("limo_stream: sequence %d (seed %llu, first tick %d): %d frames, %d keyframes, %d solves, %d landmark selections on the device, ATE rmse %.4f m (max %.4f m)\n", i,
                    (unsigned long long)d.seed, d.first_tick, ss.frames, ss.keyframes, ss.solves, driver->adjuster(i).device_selections_, ate, worst);
        char buf[768];
        // (the sequence's parameters next to its ATE: the table a sweep is run for)
        std::snprintf(buf, sizeof(buf),
                      "%s{\"seed\": %llu, \"first_tick\": %d, \"frames\": %d, \"keyframes\": %d, \"solves\": %d, \"five_point_calls\": %d, \"five_point_device_calls\": %d, "
                      "\"select_device_calls\": %d, \"depth_thres\": %.17g, \"reprojection_thres\": %.17g, \"outlier_quantile\": %.17g, \"shrubbery_weight\": %.17g, "
                      "\"window\": %d, \"ate_rmse\": %.6f, \"ate_max\": %.6f}",
                      i ? ", " : "", (unsigned long long)d.seed, d.first_tick, ss.frames, ss.keyframes, ss.solves, ss.five_point_calls, ss.five_point_device_calls,
                      driver->adjuster(i).device_selections_, sps[i].robust_loss_depth_thres, sps[i].robust_loss_reprojection_thres, sps[i].outlier_rejection_quantile,
                      sps[i].shrubbery_weight, sps[i].max_size_optimization_window, ate, worst);
        per_sequence += buf;
    }
    auto stage = [](const char* name, const LockstepDriver::Stage& s, bool last = false) {
        char buf[384];
        std::snprintf(buf, sizeof(buf), "\"%s\": {\"batched_calls\": %ld, \"items\": %ld, \"max_items\": %d, \"fallback_calls\": %ld, \"per_window_calls\": %ld, \"ms_host\": %.3f, \"ms_abi\": %.3f}%s",
                      name, s.batched_calls, s.items, s.max_items, s.fallback_calls, s.per_window_calls, 1e3 * s.sec_host, 1e3 * s.sec_abi, last ? "" : ", ");
        return std::string(buf);
    };
    std::printf("limo_stream: %d sequences in lock step on %d host threads: %d frames in %d ticks, %.2f ms per tick -> %.1f frames/s over all sequences; input synthesis %.1f ms per tick\n", N,
                driver->hostThreads(), st.frames, st.ticks, 1e3 * sec_pipeline / std::max(1, st.ticks), st.frames / sec_pipeline, 1e3 * sec_synth / std::max(1, st.ticks));
    // the JSON line (scripts/bench_lockstep.py, tests/test_lockstep_cpu.py, tests/test_gpu_lockstep.py read it): one line, the last one
    std::printf("{\"sequences\": %d, \"host_threads\": %d, \"ticks\": %d, \"frames\": %d, \"frames_per_s\": %.3f, \"ms_pipeline\": %.3f, \"ms_synthesis\": %.3f, \"stages\": {%s%s%s%s%s%s}, "
                "\"landmarks_initialised\": %ld, \"five_point_host\": %ld, \"select_host\": %ld, \"ms_host_finish\": %.3f, \"per_sequence\": [%s]}\n",
                N, driver->hostThreads(), st.ticks, st.frames, st.frames / sec_pipeline, 1e3 * sec_pipeline, 1e3 * sec_synth, stage("depth", st.depth).c_str(),
                stage("five_point", st.five_point).c_str(), stage("pose_only", st.pose_only).c_str(), stage("landmark_init", st.landmark_init).c_str(),
                stage("select", st.select).c_str(), stage("solve", st.solve, true).c_str(), st.landmarks_initialised, st.five_point_host, st.select_host, 1e3 * st.sec_host_finish,
                per_sequence.c_str());
    (void)total_frames;
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    int n_frames = 200, n_feat = 1500, n_az = 2000, window = 5, misannounce_every = 0;
    uint64_t seed = 7;
    std::string poses_path, gt_path, dump_dir, replay_dir, depth_params_path, covariance_path;
    bool use_depth = true, quiet = false, five_point_prior = false, progress = false;
    int five_point_where = -1;  // 0: host, 1: device, -1: StreamParams' default
    int select_where = -1;      // landmark selection of solve(): the same
    StreamParams::DepthAhead depth_ahead = StreamParams::DepthAhead::Thread;
    double min_flow = -1., time_between_keyframes = -1.;
    double depth_thres = -1., reprojection_thres = -1., outlier_quantile = -1., shrubbery_weight = -1.;  // (< 0: StreamParams' default)
    LockstepOptions lockstep;
    bool single_only = false;  // an option the lock-step drive does not have
    for (int i = 1; i < argc; ++i) {
        auto arg = [&](const char* name) { return !std::strcmp(argv[i], name) && i + 1 < argc; };
        if (arg("--frames")) n_frames = std::atoi(argv[++i]);
        else if (arg("--features")) n_feat = std::atoi(argv[++i]);
        else if (arg("--az")) n_az = std::atoi(argv[++i]);
        else if (arg("--seed")) seed = std::strtoull(argv[++i], nullptr, 10);
        else if (arg("--window")) window = std::atoi(argv[++i]);
        else if (arg("--sequences")) lockstep.sequences = std::atoi(argv[++i]);
        else if (arg("--frames-step")) lockstep.frames_step = std::atoi(argv[++i]);
        else if (arg("--stagger")) lockstep.stagger = std::atoi(argv[++i]);
        else if (arg("--host-threads")) lockstep.host_threads = std::atoi(argv[++i]);
        else if (arg("--perturb-rig")) lockstep.perturb_rig = std::atoi(argv[++i]);  // (testing aid, see run_lockstep)
        else if (arg("--misannounce-every")) misannounce_every = std::atoi(argv[++i]), single_only = true;  // (testing aid, see the frame loop)
        else if (arg("--perturb-trim-rounds")) lockstep.perturb_trim_rounds = std::atoi(argv[++i]);  // (testing aid, see run_lockstep)
        else if (arg("--sweep")) lockstep.sweep_path = argv[++i];
        else if (arg("--depth-thres")) depth_thres = std::atof(argv[++i]);
        else if (arg("--reprojection-thres")) reprojection_thres = std::atof(argv[++i]);
        else if (arg("--outlier-quantile")) outlier_quantile = std::atof(argv[++i]);
        else if (arg("--shrubbery-weight")) shrubbery_weight = std::atof(argv[++i]);
        else if (arg("--min-flow")) min_flow = std::atof(argv[++i]);
        else if (arg("--time-between-keyframes")) time_between_keyframes = std::atof(argv[++i]);
        else if (arg("--poses")) poses_path = argv[++i];
        else if (arg("--covariance")) covariance_path = argv[++i];
        else if (arg("--gt-poses")) gt_path = argv[++i];
        else if (arg("--dump-velodyne")) dump_dir = argv[++i], single_only = true;
        else if (arg("--velodyne")) replay_dir = argv[++i], single_only = true;
        else if (arg("--depth-params")) depth_params_path = argv[++i];
        else if (!std::strcmp(argv[i], "--no-depth")) use_depth = false;
        else if (!std::strcmp(argv[i], "--no-prefetch")) depth_ahead = StreamParams::DepthAhead::None;
        else if (arg("--depth-ahead")) {
            const std::string m = argv[++i];
            if (m != "thread" && m != "stream" && m != "none") {
                std::fprintf(stderr, "limo_stream: --depth-ahead thread|stream|none\n");
                return 2;
            }
            depth_ahead = m == "thread" ? StreamParams::DepthAhead::Thread : m == "stream" ? StreamParams::DepthAhead::Stream : StreamParams::DepthAhead::None;
        }
        else if (!std::strcmp(argv[i], "--quiet")) quiet = true;
        else if (!std::strcmp(argv[i], "--progress")) progress = single_only = true;
        else if (!std::strcmp(argv[i], "--five-point-prior")) five_point_prior = true;  // the node's prior without tf (mono_lidar.cpp:157-186)
        else if (!std::strcmp(argv[i], "--five-point-host")) five_point_where = 0;
        else if (!std::strcmp(argv[i], "--five-point-device")) five_point_where = 1;
        else if (!std::strcmp(argv[i], "--select-host")) select_where = 0;
        else if (!std::strcmp(argv[i], "--select-device")) select_where = 1;
        else {
            std::fprintf(stderr, "usage: limo_stream [--frames N] [--features N] [--az N] [--seed S] [--window K] [--min-flow px] [--time-between-keyframes sec] [--poses file] [--gt-poses file] [--dump-velodyne dir] [--velodyne dir] [--no-depth] [--depth-ahead thread|stream|none] [--depth-params file] [--five-point-prior] [--five-point-host] [--five-point-device] [--select-host] [--select-device] [--depth-thres a] [--reprojection-thres a] [--outlier-quantile q] [--shrubbery-weight w] [--quiet] [--progress] [--sequences N [--frames-step K] [--stagger S] [--host-threads T] [--sweep file]]\n");
            return 2;
        }
    }
    using clk = std::chrono::steady_clock;
    const bool in_lockstep = lockstep.sequences != 0 || lockstep.frames_step != 0 || lockstep.stagger != 0 || lockstep.host_threads != 0 || lockstep.perturb_rig >= 0 ||
                             lockstep.perturb_trim_rounds >= 0 || !lockstep.sweep_path.empty();
    if (in_lockstep && (lockstep.sequences < 1 || lockstep.frames_step < 0 || lockstep.stagger < 0 || lockstep.host_threads < 0 || single_only)) {
        std::fprintf(stderr, "limo_stream: --frames-step, --stagger, --host-threads and --sweep go with --sequences N (N >= 1, values >= 0); a lock-step drive has no --progress, "
                             "--velodyne, --dump-velodyne or --misannounce-every\n");
        return 2;
    }
    synth_world::World world(in_lockstep ? 1 : n_frames, seed);
    world.n_az = n_az;
    Camera::Ptr cam = std::make_shared<Camera>(world.f, Vector2d(world.cx, world.cy), world.cam_veh);
    StreamParams sp;
    sp.max_size_optimization_window = window;
    sp.assign_depth = use_depth;
    sp.depth_ahead = depth_ahead;
    if (depth_thres >= 0.) sp.robust_loss_depth_thres = depth_thres;
    if (reprojection_thres >= 0.) sp.robust_loss_reprojection_thres = reprojection_thres;
    if (outlier_quantile >= 0.) sp.outlier_rejection_quantile = outlier_quantile;
    if (shrubbery_weight >= 0.) sp.shrubbery_weight = shrubbery_weight;
    if (min_flow >= 0.) sp.min_median_flow = min_flow;
    if (time_between_keyframes > 0.) sp.time_between_keyframes_sec = time_between_keyframes;
    if (five_point_prior) sp.motion_prior = StreamParams::MotionPrior::FivePoint;
    if (five_point_where >= 0) sp.five_point_on_device = five_point_where == 1;
    if (select_where >= 0) sp.landmark_selection_on_device = select_where == 1;
    sp.pose_covariance = !covariance_path.empty();
    sp.solver_time_sec = -1.;  // no wall-clock cap: the drive is reproducible
    sp.image_width = (int)world.W;
    sp.image_height = (int)world.H;
    sp.height_over_ground = synth_world::World::kHeightOverGround;
    if (in_lockstep) {  // (the depths of a tick are assigned inside the tick: --depth-ahead has nothing to run ahead of)
        lockstep.n_frames = n_frames, lockstep.n_feat = n_feat, lockstep.n_az = n_az, lockstep.seed = seed;
        lockstep.poses_path = poses_path, lockstep.covariance_path = covariance_path, lockstep.gt_path = gt_path, lockstep.depth_params_path = depth_params_path, lockstep.quiet = quiet;
        return run_lockstep(lockstep, sp);
    }
    StreamDriver driver(sp, cam, world.cam_lidar);
    driver.adjuster().minimizer_progress_to_stdout_ = progress;
    if (!depth_params_path.empty()) {
        std::string err;
        if (!depth_params_yaml::load(depth_params_path, &driver.depthParams(), &err)) {
            std::fprintf(stderr, "limo_stream: --depth-params %s\n", err.c_str());
            return 2;
        }
    }

    Synth synth(world, seed, n_feat, replay_dir, dump_dir);
    double sec_synth = 0., sec_pipeline = 0.;
    size_t& n_points = synth.n_points;
    Frame frames[2];
    auto release = [&]() {
        driver.cancelPrefetch();
        for (Frame& fr : frames)
            if (fr.scan) limo_host_free(fr.scan);
    };
    auto synthesize = [&](int t, Frame& out) -> bool { return synth.frame(t, out); };
    {
        const auto t0 = clk::now();
        if (n_frames > 0 && !synthesize(0, frames[0])) {
            release();
            return 1;
        }
        sec_synth += std::chrono::duration<double>(clk::now() - t0).count();
    }
    Tracklets stale;
    for (int t = 0; t < n_frames; ++t) {
        Frame& cur = frames[t & 1];
        Frame& next = frames[(t + 1) & 1];
        const auto t0 = clk::now();
        if (t + 1 < n_frames && !synthesize(t + 1, next)) {  // the input runs one frame ahead
            release();
            return 1;
        }
        const auto t1 = clk::now();
        // --misannounce-every N (testing aid): every N-th frame the driver is told that the CURRENT frame comes next - what it prepares
        // then does not belong to the frame it gets, must be dropped, and the pose rows must not change
        if (misannounce_every > 0 && t % misannounce_every == misannounce_every - 1) {
            stale = cur.ts;
            driver.announceNextFrame(stale, cur.scan, cur.n_pts);
        } else if (t + 1 < n_frames)
            driver.announceNextFrame(next.ts, next.scan, next.n_pts);
        driver.process(std::move(cur.ts), cur.scan, cur.n_pts);  // (the tracker's message is handed over: the driver fills in depths)
        driver.waitForDepthAhead();  // (the depth thread's work on frame t+1 belongs to this timed region, not to the synthesis below)
        const auto t2 = clk::now();
        sec_synth += std::chrono::duration<double>(t1 - t0).count();
        sec_pipeline += std::chrono::duration<double>(t2 - t1).count();
        if (!quiet && (t % 100 == 0 || t == n_frames - 1)) {
            const Vector3d e = driver.poses().back().inverse().translation() - world.origin_veh[t].translation();
            std::printf("frame %d: %zu tracks, %zu points, position error %.3f m, %d keyframes, %d solves\n", t, cur.n_tracks, cur.n_pts, e.norm(),
                        driver.stats().keyframes, driver.stats().solves);
            std::fflush(stdout);
        }
    }
    release();
    // absolute trajectory error of the dumped poses (vehicle positions in the origin frame)
    double se = 0., worst = 0.;
    for (int t = 0; t < n_frames; ++t) {
        const Vector3d e = driver.poses()[t].inverse().translation() - world.origin_veh[t].translation();
        se += e.norm() * e.norm();
        worst = std::max(worst, e.norm());
    }
    const double ate = std::sqrt(se / n_frames);
    if (!poses_path.empty()) {
        std::ofstream f(poses_path);
        driver.writeKittiTrajectory(f);
    }
    if (!covariance_path.empty()) {
        std::ofstream f(covariance_path);
        driver.writeCovariances(f);
    }
    // devkit-style relative errors on the KITTI pose rows (camera frame)
    std::vector<EigenPose> gt_rows, est_rows;
    {
        const EigenPose cv = cam->getEigenPose();
        for (int t = 0; t < n_frames; ++t) {
            gt_rows.push_back(kitti_io::inCameraFrame(cv, world.origin_veh[t]));
            est_rows.push_back(kitti_io::inCameraFrame(cv, driver.poses()[t].inverse()));
        }
        if (!gt_path.empty()) {
            std::ofstream f(gt_path);
            for (const auto& p : gt_rows) kitti_io::writePoseRow(f, p);
        }
    }
    const kitti_io::TrajectoryError te = kitti_io::evaluateTrajectory(gt_rows, est_rows);
    const auto& st = driver.stats();
    std::printf("limo_stream: %d frames (%d keyframes, %d solves, window %d), %.0f points and %.0f features per frame, %.1f %% of the features with a LiDAR depth\n",
                n_frames, st.keyframes, st.solves, window, (double)n_points / n_frames, (double)st.features / n_frames,
                100. * st.features_with_depth / std::max(1, st.features));
    std::printf("limo_stream: pipeline %.2f ms per frame -> %.1f frames/s (depth %.2f, pose-only %.2f, push %.2f, solve %.2f ms per frame; %.2f ms per solve()); input synthesis %.1f ms per frame\n",
                1e3 * sec_pipeline / n_frames, n_frames / sec_pipeline, 1e3 * st.sec_depth / n_frames, 1e3 * st.sec_pose_only / n_frames,
                1e3 * st.sec_push / n_frames, 1e3 * st.sec_solve / n_frames, st.solves ? 1e3 * st.sec_solve / st.solves : 0., 1e3 * sec_synth / n_frames);
    std::printf("limo_stream: host side per frame: Keyframe object %.2f, keyframe selection %.2f, window cut + labels %.2f ms; inside the C-ABI: adjustPoseOnly %.2f of %.2f, solve %.2f of %.2f ms per frame\n",
                1e3 * st.sec_keyframe / n_frames, 1e3 * st.sec_select / n_frames, 1e3 * st.sec_window / n_frames, 1e3 * st.sec_abi_pose_only / n_frames,
                1e3 * st.sec_pose_only / n_frames, 1e3 * st.sec_abi_solve / n_frames, 1e3 * st.sec_solve / n_frames);
    std::printf("limo_stream: depth assignment one frame ahead (%s) for %d frames: %.2f ms per frame on the depth thread; per-track depth history %.3f ms per frame\n",
                depth_ahead == StreamParams::DepthAhead::Thread ? "thread" : depth_ahead == StreamParams::DepthAhead::Stream ? "stream" : "none", st.depth_prefetched,
                1e3 * st.sec_depth_thread / n_frames, 1e3 * st.sec_depth_history / n_frames);
    std::printf("limo_stream: ATE rmse %.4f m (max %.4f m) over %.1f m\n", ate, worst, 0.55 * (n_frames - 1));
    if (te.rel_samples)
        std::printf("limo_stream: relative errors over 100..800 m sub-paths (KITTI devkit measure, %d samples): translation %.3f %%, rotation %.5f deg/m\n",
                    te.rel_samples, 100. * te.rel_trans, te.rel_rot * 180. / M_PI);
    std::printf("frames %d\nfps %.3f\nate_rmse %.6f\nate_max %.6f\ndepth_fraction %.4f\nkeyframes %d\nsolves %d\nsolves_on_non_keyframes %d\ndepth_prefetched %d\n", n_frames,
                n_frames / sec_pipeline, ate, worst, (double)st.features_with_depth / std::max(1, st.features), st.keyframes, st.solves, st.solves_on_non_keyframes,
                st.depth_prefetched);
    std::printf("select_device_calls %d\n", driver.adjuster().device_selections_);
    if (five_point_prior)
        std::printf("limo_stream: five-point prior: %d estimates (%d on the device), %.3f ms each\nfive_point_calls %d\nfive_point_device_calls %d\nfive_point_ms %.4f\n",
                    st.five_point_calls, st.five_point_device_calls, st.five_point_calls ? 1e3 * st.sec_five_point / st.five_point_calls : 0., st.five_point_calls,
                    st.five_point_device_calls, st.five_point_calls ? 1e3 * st.sec_five_point / st.five_point_calls : 0.);
    return 0;
}
