"""Narrow ground-plane Schur waves (kba_kernels.hip:k_schur_lean_gp, schur_lean_group<2, true, false, true>) against the
three-panel waves, bit for bit.

A ground-plane group whose rows all hang on one keyframe (SchurGroup::gp_class, decided at pack time) builds a two-panel tile - pose
columns, rhs, that keyframe's plane slots - and stores +0.0 to the slab entries of the other plane slots.  Every case is solved as a
batch twice in one process - default, and after a reset under KBA_SCHUR_GP_WIDE=1 (every group through the three-panel kernel) - and
both are compared with the same windows solved one per call: everything limo_ba_batch_download returns, the trimmed sets and the
per-iteration log must be byte-equal.  limo_ctx_last_schur_gp_info has to show that narrow waves ran in the default solve and did
not run in the forced-wide one; a case where it cannot tell fails.

Shapes (5 keyframes x 200 landmarks of synth.make_window before its selection; keyframe 0 is Pose-fixed, so four keyframes are free
and the ground-plane tile has 41 columns, three panels):
  (a) 35 ground rows, all on the newest keyframe: one group of two full tiles and a partial one;
  (b) 65 .. 79 ground rows: blocks of 64 + a few, the second group is one tile with idle lanes;
  (c) a mixed batch: (a); (a) with the newest keyframe's plane invalid (kf_plane_dist < -10), all rows on the keyframe before it;
      the same with the two newest invalid - rows on keyframe 2, whose plane columns straddle the boundary of the second and third
      panel of the wide tile; and (a) with five ground landmarks moved beside keyframe 1: a wide group, both kinds of wave in one
      launch.
      The edited windows are for bit equality only;
  (d) (a) next to (a) with the newest keyframe Pose-fixed: its rows hang on a keyframe without a free plane slot (class -1);
  (e) windows of 3 and 4 keyframes: two panels, nothing is classified, the narrow kernel never runs.
Paths: the lock-step launches, the streaming solve (so few windows that every round is a draining round: the pair kernel, whose
ground-plane waves pick their tile by the record as well) and the streaming solve without the pair kernel.
Oracle parity of the default batch solve on (a), (b) and (d) at the tolerance of tests/test_gpu_ba.py.
"""
import numpy as np
import pytest

from limo_amd import _ffi, ba, default_options, synth
from test_gpu_ba import TOL, rel_pose_err

pytestmark = pytest.mark.gpu

A = dict(seed=9100, n_kf=5, n_lm=200, ground_frac=0.4)   # 35 ground landmarks within 25 m of a keyframe: the rows
B = dict(seed=9105, n_kf=5, n_lm=200, ground_frac=0.75)  # 71 rows: blocks of 64 + 7
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "n_depth_blocks", "n_repr_blocks",
               "n_gp_blocks", "n_trimmed_landmarks", "num_linearizations", "initial_cost", "final_cost")
_ENV = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_NO_SCHUR_PAIR", "KBA_SCHUR_GP_WIDE")
PATHS = {
    "lockstep": ({"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}, "LOCKSTEP"),
    "streaming_pair": ({"KBA_STREAM_MIN": "1"}, "STREAMING"),
    "streaming": ({"KBA_STREAM_MIN": "1", "KBA_NO_SCHUR_PAIR": "1"}, "STREAMING"),
}


def _kf_position(w, k):
    R, t = synth.pose_to_Rt(w.kf_pose[k])
    return -R.T @ t


def row_keyframes(w):
    """Keyframe each ground landmark's row hangs on, or -1 (kba_pack.cpp: the nearest keyframe with a valid plane, within 25 m)."""
    out = -np.ones(w.n_lm, np.int64)
    best = np.full(w.n_lm, np.inf)
    for k in range(w.n_kf):
        if w.kf_plane_dist[k] < -10.0:
            continue
        R, t = synth.pose_to_Rt(w.kf_pose[k])
        d = np.linalg.norm(w.lm_pos @ R.T + t, axis=1)
        closer = d < best
        best[closer], out[closer] = d[closer], k
    out[(best >= 25.0) | (w.lm_is_ground == 0)] = -1
    return out


def _a():
    return synth.make_window(**A)


def _a_planes_invalid(n):
    w = _a()
    w.kf_plane_dist = w.kf_plane_dist.copy()
    w.kf_plane_dist[w.n_kf - n:] = -11.0
    return w


def _a_moved():
    w = _a()
    g = np.flatnonzero(row_keyframes(w) == w.n_kf - 1)[:5]
    w.lm_pos = w.lm_pos.copy()
    for j, l in enumerate(g):  # to the left of keyframe 1 (the keyframes are about 4 m apart along x), half a metre from each other
        w.lm_pos[l] = _kf_position(w, 1) + np.array([0.2 * j - 0.4, 2.0 + 0.5 * j, -synth.HEIGHT_OVER_GROUND])
    return w


def _a_newest_fixed():
    w = _a()
    w.kf_fixation = w.kf_fixation.copy()
    w.kf_fixation[-1] = _ffi.LIMO_FIX_POSE
    return w


# name -> (windows, narrow groups, wide groups the pack has to count)
def _cases():
    return {
        "a": ([_a()], 1, 0),
        "b": ([synth.make_window(**B)], 2, 0),
        "c": ([_a(), _a_planes_invalid(1), _a_planes_invalid(2), _a_moved()], 3, 1),
        "d": ([_a(), _a_newest_fixed()], 2, 0),
        "e": ([synth.make_window(9102, n_kf=3, n_lm=200), synth.make_window(9103, n_kf=4, n_lm=200)], 0, 0),
    }


def _result(b, reps, i):
    w = b.windows[i]
    return (tuple(reps[i][k] for k in REPORT_KEYS), w.kf_pose.tobytes(), w.kf_plane_dir.tobytes(), w.kf_plane_dist.tobytes(), w.lm_pos.tobytes(),
            b.trimmed(i).tobytes(), b.iteration_log(i).tobytes())


def _same(a, b, what):
    assert a[0] == b[0], (what, dict(zip(REPORT_KEYS, a[0])), dict(zip(REPORT_KEYS, b[0])))
    for name, x, y in zip(("kf_pose", "kf_plane_dir", "kf_plane_dist", "lm_pos", "trimmed", "iteration_log"), a[1:], b[1:]):
        assert x == y, (what, name)
    assert len(a[6]) > 0 and np.isfinite(np.frombuffer(a[1])).all() and np.isfinite(np.frombuffer(a[4])).all(), what


_cache = {}  # windows and their one-per-call results: computed once, shared, never changed


def _setenv(monkeypatch, env):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _reference(ctx, name, monkeypatch):
    """The windows of a case solved one per call (a batch of one window each, the default path)."""
    if name not in _cache:
        _setenv(monkeypatch, {})
        windows = _cases()[name][0]
        out = []
        for w in windows:
            b = ba.Batch(ctx, [w.copy()])
            b.solve(default_options())
            out.append(_result(b, b.download(), 0))
            b.close()
        _cache[name] = (windows, out)
    return _cache[name]


def _run(ctx, name, path, monkeypatch):
    env, want_path = PATHS[path]
    _, n_narrow, n_wide = _cases()[name]
    ctx.set_iteration_log(True)
    try:
        windows, ref = _reference(ctx, name, monkeypatch)
        _setenv(monkeypatch, env)  # (KBA_NO_SCHUR_PAIR is read when the batch is made)
        b = ba.Batch(ctx, [w.copy() for w in windows])
        got = {}
        for forced in (False, True):
            _setenv(monkeypatch, dict(env, KBA_SCHUR_GP_WIDE="1") if forced else env)
            b.reset()
            b.solve(default_options())
            reps = b.download()
            info, gp = ctx.last_solve_info(), ctx.last_schur_gp_info()
            assert info["path"] == want_path and info["recovered"] == 0, (name, path, forced, info)
            assert (gp["narrow_groups"], gp["wide_groups"]) == (n_narrow, n_wide), (name, path, forced, gp)
            pair = info["pair_launches"] > 0
            assert pair == (path == "streaming_pair"), (name, path, info)
            if forced or n_narrow == 0:
                assert gp["narrow_launches"] == 0 and gp["wide_launches"] > 0, (name, path, forced, gp)
            else:
                assert gp["narrow_launches"] > 0 and (gp["wide_launches"] > 0) == (n_wide > 0), (name, path, gp)
            got[forced] = [_result(b, reps, i) for i in range(len(windows))]
        b.close()
    finally:
        _setenv(monkeypatch, {})
        ctx.set_iteration_log(False)
    for forced in (False, True):
        for i in range(len(windows)):
            _same(ref[i], got[forced][i], (name, path, "forced wide" if forced else "default", i))
    return windows, got[False]


def test_shapes_are_what_the_cases_are_for():
    a = _a()
    ra = row_keyframes(a)
    n = int((ra >= 0).sum())
    assert a.n_kf == 5 and 33 <= n <= 47 and (ra[ra >= 0] == 4).all(), (n, np.bincount(ra[ra >= 0]))
    b = synth.make_window(**B)
    rb = row_keyframes(b)
    assert 65 <= (rb >= 0).sum() <= 79 and (rb[rb >= 0] == 4).all(), (rb >= 0).sum()
    for k, w in ((3, _a_planes_invalid(1)), (2, _a_planes_invalid(2))):
        r = row_keyframes(w)
        assert 16 < (r >= 0).sum() <= 64 and (r[r >= 0] == k).all(), (k, np.bincount(r[r >= 0]))
    r = row_keyframes(_a_moved())
    assert (r == 1).sum() == 5 and (r == 4).sum() == n - 5 and n <= 64  # two keyframes inside one block
    assert (a.obs_d > 0).sum() >= 10  # four free plane slots per keyframe (kba_pack.cpp): keyframe 2's sit in columns 29 .. 32
    rd = row_keyframes(_a_newest_fixed())
    assert np.array_equal(rd, ra)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["a", "c"])
def test_narrow_equals_wide_equals_one_per_call(ctx, name, path, monkeypatch):
    _run(ctx, name, path, monkeypatch)


@pytest.mark.parametrize("name", ["e"])
def test_two_panel_batches_stay_as_they_are(ctx, name, monkeypatch):
    _run(ctx, name, "lockstep", monkeypatch)


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_oracle_parity_of_the_narrow_solve(ctx, oracle, name, monkeypatch):
    windows, got = _run(ctx, name, "lockstep", monkeypatch)
    opts = default_options()
    for w, g in zip(windows, got):
        wo = w.copy()
        ro, _ = oracle.solve(wo, opts)
        rg = dict(zip(REPORT_KEYS, g[0]))
        pose = np.frombuffer(g[1]).reshape(-1, 7)
        assert rg["n_depth_blocks"] == ro["n_depth_blocks"] and rg["n_gp_blocks"] == ro["n_gp_blocks"]
        assert rg["n_trimmed_landmarks"] == ro["n_trimmed_landmarks"]
        assert abs(rg["initial_cost"] - ro["initial_cost"]) <= 1e-9 * abs(ro["initial_cost"])
        assert abs(rg["final_cost"] - ro["final_cost"]) <= TOL * abs(ro["final_cost"])
        assert rel_pose_err(pose, wo.kf_pose) <= TOL
        assert np.array_equal(pose[0], w.kf_pose[0])  # keyframe 0 is Pose-fixed: bit-identical
