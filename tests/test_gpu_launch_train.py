"""One launch train for an LM iteration: what every launch path of the solve shares since the lock-step sequence runs the kernels of
the streaming solve (k_step_decide moves the accepted keyframes on every path, the relinearisation moves the accepted landmarks,
k_after_step damps again after a rejected step).

Two properties the other GPU tests do not pin down: a window WITHOUT landmark workgroups whose keyframes really move, and a solve
with many rejected steps - consecutive ones among them - on every launch path.
"""
import os

import numpy as np
import pytest

from limo_amd import ba, default_options, synth
from limo_amd.window import Window

pytestmark = pytest.mark.gpu

_ENV = ("KBA_NO_WG_SOLVE", "KBA_NO_COOP_SOLVE", "KBA_STREAM_MIN")
REPORT_KEYS = ("final_cost", "initial_cost", "iterations_total", "iterations_final", "num_solves", "n_trimmed_landmarks", "termination",
               "successful_steps", "num_linearizations")


def _set_env(monkeypatch, env):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _bare_pose_only_case():
    """synth.make_pose_only_case(71) without any landmark or observation: the speed prior is the only residual block, so the window
    has no landmark workgroup at all - and the prior pulls the pose away from where it starts."""
    pw, prior, _ = synth.make_pose_only_case(71)
    bare = Window(**{n: (getattr(pw, n)[:0] if (n.startswith("obs_") or n.startswith("lm_")) else getattr(pw, n)) for n, _ in Window.FIELDS})
    return bare, prior


def test_window_without_landmarks_whose_pose_moves(ctx, oracle, monkeypatch):
    """The accepted keyframes of a window without landmark workgroups move through k_step_decide alone (no landmark pass ever sees
    the window).  The CPU emulator takes 4 iterations, 3 of them successful, on this window and moves the pose by 0.20; the oracle ends
    within 4e-13 of it.  (The final cost is ~1e-19: not compared relatively.)"""
    bare, prior = _bare_pose_only_case()
    o = default_options(min_landmarks_for_trimming=30)
    po = bare.copy()
    oracle.adjust_pose_only(po, prior, o)
    runs = []
    for env, path in (({}, "WG"), ({"KBA_NO_WG_SOLVE": "1"}, "COOP"), ({"KBA_NO_WG_SOLVE": "1", "KBA_NO_COOP_SOLVE": "1"}, "LOCKSTEP")):
        _set_env(monkeypatch, env)
        x = bare.copy()
        runs.append((x, ctx.adjust_pose_only(x, prior, o)))
        assert ctx.last_solve_info()["path"] == path
    _set_env(monkeypatch, {})
    a, ra = runs[0]
    for b, rb in runs[1:]:
        assert a.kf_pose.tobytes() == b.kf_pose.tobytes()
        for k in REPORT_KEYS:
            assert ra[k] == rb[k], (k, ra[k], rb[k])
    moved = np.abs(a.kf_pose - bare.kf_pose).max()
    err = np.abs(a.kf_pose - po.kf_pose).max()
    print("iterations %d, successful steps %d, pose moved by %.3g, |pose - oracle| %.3g, final cost %.3g"
          % (ra["iterations_total"], ra["successful_steps"], moved, err, ra["final_cost"]))
    assert ra["iterations_total"] >= 3 and ra["successful_steps"] >= 2
    assert moved > 0.1
    assert err <= 1e-6  # the bar of test_pose_only_matches_oracle
    # second of three in a pose-only batch on the lock-step sequence (KBA_NO_WG_SOLVE=1): the bytes of its single call
    others = [synth.make_pose_only_case(72), synth.make_pose_only_case(73)]
    wins = [others[0][0].copy(), bare.copy(), others[1][0].copy()]
    priors = [others[0][1], prior, None]
    _set_env(monkeypatch, {"KBA_NO_WG_SOLVE": "1"})
    bt = ba.Batch(ctx, wins, pose_only=True, priors=priors)
    bt.solve(o)
    assert ctx.last_solve_info()["path"] == "LOCKSTEP"
    reps = bt.download()
    launches = bt.kernel_stats()["linearize_launches"]
    bt.close()
    _set_env(monkeypatch, {})
    assert launches > 0  # (only the lock-step sequence times its linearisation launches)
    assert bt.windows[1].kf_pose.tobytes() == a.kf_pose.tobytes()
    for k in REPORT_KEYS:
        assert reps[1][k] == ra[k], (k, reps[1][k], ra[k])


def test_rejected_steps_on_every_launch_path(ctx, monkeypatch):
    """tests/golden/window_drive_frame1674.npz (about 60 iterations, 13 rejected steps, consecutive ones among them): as one window
    through the one-launch solve, as one window through the lock-step sequence, as a batch of two copies through the streaming solve -
    the same poses, planes, landmarks, trimmed sets and reports.  The CPU emulator counts 66 iterations and 49 successful steps on this
    window, iterations_total - successful_steps = 17; >= 5 here, so that the test cannot pass without the re-damping after a
    rejected step having run."""
    import window_io

    w = window_io.load_npz(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_drive_frame1674.npz"))
    o = default_options()
    results = []  # (what, window, report, trimmed set)
    for what, env, n, path in (("one launch", {}, 1, "COOP"), ("lock-step", {"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}, 1, "LOCKSTEP"),
                               ("streaming", {"KBA_STREAM_MIN": "1"}, 2, "STREAMING")):
        _set_env(monkeypatch, env)
        b = ba.Batch(ctx, [w.copy() for _ in range(n)])
        b.solve(o)
        info = ctx.last_solve_info()
        assert info["path"] == path and info["recovered"] == 0, (what, info)
        reps = b.download()
        for i in range(n):
            results.append(("%s, window %d" % (what, i), b.windows[i], reps[i], b.trimmed(i)))
        b.close()
    _set_env(monkeypatch, {})
    assert len(results) == 4
    _, wa, ra, ta = results[0]
    for what, wb, rb, tb in results[1:]:
        assert wa.kf_pose.tobytes() == wb.kf_pose.tobytes(), what
        assert wa.kf_plane_dir.tobytes() == wb.kf_plane_dir.tobytes() and wa.kf_plane_dist.tobytes() == wb.kf_plane_dist.tobytes(), what
        assert wa.lm_pos.tobytes() == wb.lm_pos.tobytes(), what
        assert np.array_equal(ta, tb), what
        for k in REPORT_KEYS:
            assert ra[k] == rb[k], (what, k, ra[k], rb[k])
    print("iterations %d, successful steps %d" % (ra["iterations_total"], ra["successful_steps"]))
    assert ra["iterations_total"] - ra["successful_steps"] >= 5
