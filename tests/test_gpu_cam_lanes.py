"""The 128-lane form of the camera kernels (k_cam_assemble<128>, k_cam_solve<128>: limo_amd/csrc/kba_items.hpp, cam_assemble / cam_solve
with 128 lanes that stand in for 256 virtual ones) on the GPU: a batch solved under KBA_CAM_LANES=128 and under KBA_CAM_LANES=256, on
the streaming and on the lock-step path, gives the same reports and the same parameter bytes, and the bytes of the one-launch paths
(k_solve_coop, k_solve_wg), which keep 256 lanes.  limo_ctx_last_cam_lanes_info has to show that the 128-lane launches really ran; a
case where it cannot tell fails.

Batches of 16 - 18 windows, the smallest shapes that reach every place of the two functions that depends on the lane count:
2 keyframes (the last pivot block of the Cholesky has two pivots, no trailing tile) and 5 keyframes (three tile rows, more keyframes
than waves for the Gram tile and the Cholesky's tiles dealt over two waves) with 60 - 200 landmarks; windows of 2000 landmarks (more
than 128 ground-plane rows: the staging takes a second chunk, the second virtual lane of a lane has rows of its own in the sums); a
window whose first step is rejected (the solve reads the undamped hand-over twice); constant landmarks (the fixed-cost branch of the
reductions); and a batch with a 12-keyframe window (camera system in global memory), which has to keep 256 lanes under
KBA_CAM_LANES=128 and its bytes."""
import numpy as np
import pytest

from limo_amd import ba, default_options, synth

pytestmark = pytest.mark.gpu

PATH_SWITCHES = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_COOP_MAX_WIN", "KBA_GROUPS", "KBA_COOP_TIMEOUT_MS", "KBA_CAM_LANES")
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "num_linearizations",
               "n_depth_blocks", "n_repr_blocks", "n_gp_blocks", "n_trimmed_landmarks", "initial_cost", "final_cost")


def _force(monkeypatch, path, lanes):
    for k in PATH_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if path in ("STREAMING", "LOCKSTEP"):
        monkeypatch.setenv("KBA_NO_COOP_SOLVE", "1")
        monkeypatch.setenv("KBA_NO_WG_SOLVE", "1")
        monkeypatch.setenv("KBA_STREAM_MIN", "1" if path == "STREAMING" else "100000")
    elif path == "COOP":
        monkeypatch.setenv("KBA_NO_WG_SOLVE", "1")
    if lanes:
        monkeypatch.setenv("KBA_CAM_LANES", str(lanes))


def _state(b, reps):
    return [(tuple(r[k] for k in REPORT_KEYS), w.kf_pose.tobytes(), w.kf_plane_dir.tobytes(), w.kf_plane_dist.tobytes(), w.lm_pos.tobytes())
            for w, r in zip(b.windows, reps)]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], (what, i, dict(zip(REPORT_KEYS, x[0])), dict(zip(REPORT_KEYS, y[0])))
        assert x[1:] == y[1:], (what, i)


def _solve(ctx, monkeypatch, path, lanes, windows, lm_fixed=None, opts=None):
    """... on `path` with KBA_CAM_LANES=`lanes` (None: unset): state, reports and the lanes the camera launches took"""
    _force(monkeypatch, path, lanes)
    b = ba.Batch(ctx, [w.copy() for w in windows], lm_fixed=lm_fixed)
    b.solve(opts or default_options())
    info, cam = ctx.last_solve_info(), ctx.last_cam_lanes_info()
    assert info["path"] == path and info["recovered"] == 0, info
    reps = b.download()
    st = _state(b, reps)
    b.close()
    return st, reps, cam


def _took(cam, lanes):
    """every camera launch of the solve took `lanes` lanes, and there were some"""
    other = 384 - lanes
    return (cam["assemble_%d" % lanes] > 0 and cam["solve_%d" % lanes] > 0 and cam["assemble_%d" % other] == 0 and cam["solve_%d" % other] == 0)


def _both_forms_on_both_paths(ctx, monkeypatch, ws, lm_fixed=None, opts=None):
    """128 and 256 lanes on the lock-step and the streaming path: one state; returns it with the reports"""
    want, reps, cam = _solve(ctx, monkeypatch, "LOCKSTEP", 256, ws, lm_fixed, opts)
    assert _took(cam, 256) and cam["global_class_windows"] == 0, cam
    for path, lanes in (("LOCKSTEP", 128), ("STREAMING", 128), ("STREAMING", 256)):
        st, _, cam = _solve(ctx, monkeypatch, path, lanes, ws, lm_fixed, opts)
        assert _took(cam, lanes), (path, lanes, cam)
        _assert_same(st, want, "%s, %d lanes" % (path, lanes))
    return want, reps


def _windows(n, kfs, seed0):
    return [synth.make_window(seed0 + i, n_kf=kfs[i % len(kfs)], n_lm=60 + (37 * i) % 141) for i in range(n)]


def test_two_and_five_keyframes_same_bytes_as_the_cooperative_solve(ctx, monkeypatch):
    ws = _windows(16, (2, 5), 9100)
    want, reps = _both_forms_on_both_paths(ctx, monkeypatch, ws)
    assert any(r["iterations_total"] > 2 for r in reps)
    st, _, cam = _solve(ctx, monkeypatch, "COOP", 128, ws)  # (one launch: no camera launch to pick a form for)
    assert sum(cam[k] for k in ("assemble_128", "assemble_256", "solve_128", "solve_256")) == 0, cam
    _assert_same(st, want, "COOP")
    # the rule on its own: 16 windows are one pass of either form - 256 lanes
    st, _, cam = _solve(ctx, monkeypatch, "STREAMING", None, ws)
    assert _took(cam, 256), cam
    _assert_same(st, want, "STREAMING, the rule")
    # ... and the instances are what the plan counts on: twice the workgroups per compute unit, or the rule never picks the form
    print("workgroups per CU", cam)
    assert cam["wg_per_cu_assemble_128"] >= 2 * cam["wg_per_cu_assemble_256"] >= 2, cam
    assert cam["wg_per_cu_solve_128"] >= 2 * cam["wg_per_cu_solve_256"] >= 2, cam


def test_more_than_128_ground_plane_rows(ctx, monkeypatch):
    ws = _windows(16, (5, 2), 9200)
    for i in (0, 5, 10):  # 5, 2 and 5 keyframes
        ws[i] = synth.make_window(9200 + i, n_kf=ws[i].n_kf, n_lm=2000)  # (880 landmarks leave 67 - 88 ground-plane rows)
    want, reps = _both_forms_on_both_paths(ctx, monkeypatch, ws)
    print("ground-plane rows", [r["n_gp_blocks"] for r in reps])
    assert sum(r["n_gp_blocks"] > 128 for r in reps) >= 2, [r["n_gp_blocks"] for r in reps]  # from the report, not from the generator


def test_rejected_first_step(ctx, monkeypatch):
    """min_relative_decrease = 4 rejects the first step of these windows (tests/test_gpu_cam_handover.py): the next iteration solves
    the same linearisation with a smaller radius, from the hand-over of the one assembly."""
    ws = [synth.make_window(8400 + i, n_kf=(5, 2)[i % 2], n_lm=60 + (37 * i) % 141) for i in range(16)]
    o = default_options(min_relative_decrease=4.0)
    want, reps = _both_forms_on_both_paths(ctx, monkeypatch, ws, opts=o)
    # (a rejected step costs an iteration and no linearisation)
    again = [i for i, r in enumerate(reps) if r["num_linearizations"] < r["iterations_total"] + r["num_solves"] and r["successful_steps"] > 0]
    print("a step rejected, a later one accepted, in windows", again)
    assert again, "no window solved a linearisation twice and moved afterwards"


def test_constant_landmarks_same_bytes_as_the_workgroup_solve(ctx, monkeypatch):
    ws = _windows(16, (2, 5), 9300)
    # every third landmark constant: fixed-cost pairs and ground rows next to variable ones (the reg_fixed sums)
    flags = [(np.arange(w.n_lm) % 3 == 0).astype(np.uint8) for w in ws]
    want, reps = _both_forms_on_both_paths(ctx, monkeypatch, ws, lm_fixed=flags)
    assert any(r["iterations_total"] > 2 for r in reps)
    # every landmark constant: no Schur block, k_solve_wg (256 lanes) serves the batch
    flags = [np.ones(w.n_lm, np.uint8) for w in ws]
    want, reps = _both_forms_on_both_paths(ctx, monkeypatch, ws, lm_fixed=flags)
    assert any(r["iterations_total"] > 1 for r in reps)
    st, _, cam = _solve(ctx, monkeypatch, "WG", 128, ws, lm_fixed=flags)
    _assert_same(st, want, "WG")


def test_a_global_memory_window_keeps_the_batch_at_256_lanes(ctx, monkeypatch):
    ws = _windows(17, (2, 5), 9400)
    ws[7] = synth.make_window(9407, n_kf=12, n_lm=160)
    want, _, cam = _solve(ctx, monkeypatch, "LOCKSTEP", 256, ws)
    assert _took(cam, 256), cam
    for path in ("LOCKSTEP", "STREAMING"):
        st, _, cam = _solve(ctx, monkeypatch, path, 128, ws)
        # the 12-keyframe window, and nothing else, is of the global-memory class ...
        assert cam["global_class_windows"] == 1, cam
        # ... and it alone is why the batch keeps 256 lanes: the LDS sizes are those of the 5-keyframe windows, at which the 128-lane
        # instances double the workgroups per compute unit
        assert cam["wg_per_cu_assemble_128"] >= 2 * cam["wg_per_cu_assemble_256"] >= 2, cam
        assert cam["wg_per_cu_solve_128"] >= 2 * cam["wg_per_cu_solve_256"] >= 2, cam
        assert _took(cam, 256), (path, cam)  # zero 128-lane launches
        _assert_same(st, want, path)
    # the same batch without that window takes 128 lanes: the 256-lane instances worked in global memory next to windows that could
    del ws[7]
    st, _, cam = _solve(ctx, monkeypatch, "STREAMING", 128, ws)
    assert cam["global_class_windows"] == 0 and _took(cam, 128), cam
    _assert_same(st, want[:7] + want[8:], "without the 12-keyframe window")
