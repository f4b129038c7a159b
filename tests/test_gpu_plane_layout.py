"""The two plane scalars of a pair live at the pair's own index (kba_layout.hpp:BatchView::obs_c): plane k of (view j of its window,
packed landmark gl) at k * stride + j * SL + gl, the index of the pair's entry in lm_slot.  k_lin_lm writes every pair of the views with
a free pose block, +0.0 where the landmark has no observation in the view; the Schur waves and the back-substitution load the planes at
an address they know from the window's record and the lane alone, and the slot only decides whether the loaded value counts.

Windows - the smallest at which that addressing can go wrong, synth.make_window cut to an exact number of landmarks with observations
deleted (a Schur block is 64 landmarks of one class, a tile 16, a plain group two blocks, a ground-plane group one):
  (a) 3 keyframes x 17 landmarks: one full tile plus one lane;
  (b) 3 x 65: one landmark past a block, all plain - and 4 x 65 with ground-plane landmarks only (the lean ground-plane waves; four
      keyframes because the unobserved free keyframe of the "noview" variant keeps its pose block through the ground-plane
      regularisers: with three keyframes nothing determines its translation, and the window would fail the parity bar for a reason
      of its own - the oracle and the solve end at the same cost with different translations of that keyframe);
  (c) 3 x 130: one tile past a two-block group;
  (d) a stereo window (two views per keyframe: k_schur_wide, kba_items.hpp:schur_pair_block);
  (e) a 2-keyframe and a 6-keyframe window in one batch: the plane rows beyond a window's own views exist and are never touched.
Every shape comes twice.  "sparse": one landmark is observed only by the pose-fixed first keyframe and one free keyframe, the last
landmark of every block is missing in the last view, every fifth landmark misses one free view.  "noview": one free view has no
observation at all (its plane rows hold nothing but the +0.0 of the writer).  The trimming options make at least one window lose
landmarks in its trimming round (their lanes then store +0.0 in every view).

Assertions: every window within the parity bar of tests/test_gpu_ba.py against the oracle (<= 1e-4 on final cost and translations); the
streaming, lock-step and one-launch paths give the same bytes (the one-launch kernel takes fast-class windows: not (d), not the
6-keyframe window); a streaming solve in a process of its own under KBA_POISON=1 gives the bytes of the unpoisoned one.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from limo_amd import ba, default_options, synth  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the parity bar of tests/test_gpu_ba.py
# gen: landmarks asked of synth.make_window (its selection drops some), n_lm: landmarks kept
SHAPES = [
    dict(name="a", seed=8101, n_kf=3, gen=60, n_lm=17, with_ground_plane=False),
    dict(name="b", seed=8102, n_kf=3, gen=160, n_lm=65, with_ground_plane=False),
    dict(name="b_ground", seed=8103, n_kf=4, gen=160, n_lm=65, ground_frac=1.0),
    dict(name="c", seed=8104, n_kf=3, gen=300, n_lm=130, with_ground_plane=False),
    dict(name="d_stereo", seed=8105, n_kf=3, gen=160, n_lm=65, stereo_baseline=0.54),
    dict(name="e_2kf", seed=8106, n_kf=2, gen=120, n_lm=40),
    dict(name="e_6kf", seed=8107, n_kf=6, gen=200, n_lm=70),
]
VARIANTS = ("sparse", "noview")
CASES = [(s, v) for s in SHAPES for v in VARIANTS if not (s["n_kf"] == 2 and v == "noview")]  # (two keyframes: one free view)
FAST = [i for i, (s, _) in enumerate(CASES) if s["name"] not in ("d_stereo", "e_6kf")]  # windows the one-launch kernel takes
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "n_depth_blocks", "n_repr_blocks",
               "n_gp_blocks", "n_trimmed_landmarks", "num_linearizations", "initial_cost", "final_cost")
_ENV = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_NO_SCHUR_PAIR", "KBA_GROUPS", "KBA_COOP_MAX_WIN")
LOCK_STEP = {"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1", "KBA_STREAM_MIN": "100000"}
STREAMING = {"KBA_STREAM_MIN": "1"}


def options():
    """Trimming reaches windows of 17 landmarks (the defaults start at 100 landmarks / 30 residual groups)."""
    return default_options(min_landmarks_for_trimming=10, minimum_number_residual_groups=10)


def _cut(w, keep_obs, n_lm=None):
    for name in ("obs_kf", "obs_lm", "obs_cam", "obs_u", "obs_v", "obs_d"):
        setattr(w, name, np.ascontiguousarray(getattr(w, name)[keep_obs]))
    if n_lm is not None:
        for name in ("lm_pos", "lm_weight", "lm_is_ground"):
            setattr(w, name, np.ascontiguousarray(getattr(w, name)[:n_lm]))
    w.validate()


def views_of(w):
    return w.obs_kf.astype(np.int64) * w.n_cam + w.obs_cam


def make_case(shape, variant):
    kw = {k: v for k, v in shape.items() if k not in ("name", "seed", "gen", "n_lm")}
    w = synth.make_window(shape["seed"], n_lm=shape["gen"], **kw)
    # the first n_lm landmarks that the first two keyframes both see (camera 0): every deletion below leaves them two observations
    seen01 = np.zeros((2, w.n_lm), bool)
    m = (w.obs_kf < 2) & (w.obs_cam == 0)
    seen01[w.obs_kf[m], w.obs_lm[m]] = True
    good = np.flatnonzero(seen01.all(axis=0))
    assert good.size >= shape["n_lm"], (shape, good.size)
    good = good[: shape["n_lm"]]
    new = -np.ones(w.n_lm, np.int64)
    new[good] = np.arange(good.size)
    keep = new[w.obs_lm] >= 0
    w.obs_lm = new[w.obs_lm].astype(np.int32)
    for name in ("lm_pos", "lm_weight", "lm_is_ground"):
        setattr(w, name, np.ascontiguousarray(getattr(w, name)[good]))
    _cut(w, keep)
    n = w.n_lm
    last_view = w.n_kf * w.n_cam - 1
    v = views_of(w)
    protected = (w.obs_kf < 2) & (w.obs_cam == 0)  # keyframe 0 (pose-fixed) and keyframe 1 (free), camera 0: never deleted
    drop = np.zeros(w.n_obs, bool)
    if variant == "sparse":
        drop |= (w.obs_lm == 0) & ~protected                                  # landmark 0: the fixed keyframe and ONE free keyframe
        ends = np.array(sorted({min(n, b + 64) - 1 for b in range(0, n, 64)}))
        drop |= np.isin(w.obs_lm, ends) & (v == last_view) & ~protected       # the last landmark of every block, in the last view
        free_views = np.arange(2 * w.n_cam, w.n_kf * w.n_cam)                 # views behind the protected keyframes
        if free_views.size:
            drop |= (w.obs_lm % 5 == 3) & (v == free_views[(w.obs_lm // 5) % free_views.size]) & ~protected
    else:
        drop |= v == last_view                                                # a free view with no observation at all
    _cut(w, ~drop)
    return w


def check_not_degenerate(w, variant):
    """Every landmark keeps two observations; every keyframe that is observed at all keeps enough for its pose block."""
    assert np.bincount(w.obs_lm, minlength=w.n_lm).min() >= 2
    per_kf = np.bincount(w.obs_kf, minlength=w.n_kf)
    assert all(c == 0 or c >= 10 for c in per_kf), per_kf
    if variant == "noview":
        assert (views_of(w) == w.n_kf * w.n_cam - 1).sum() == 0


def _result(b, reps, i):
    w = b.windows[i]
    return (tuple(reps[i][k] for k in REPORT_KEYS), w.kf_pose.tobytes(), w.kf_plane_dir.tobytes(), w.kf_plane_dist.tobytes(), w.lm_pos.tobytes(),
            b.trimmed(i).tobytes())


def _digest(r):
    h = hashlib.sha256(repr(r[0]).encode())
    for x in r[1:]:
        h.update(x)
    return h.hexdigest()


def _solve_batch(ctx, windows):
    b = ba.Batch(ctx, [w.copy() for w in windows])
    b.solve(options())
    reps = b.download()
    out = [_result(b, reps, i) for i in range(len(windows))]
    b.close()
    return out


_cache = {}  # windows and results computed once, shared, never changed


def windows():
    if "windows" not in _cache:
        _cache["windows"] = [make_case(s, v) for s, v in CASES]
    return _cache["windows"]


def _solve(ctx, ws, monkeypatch, env, path):
    """... under `env`; `path`: the launch path the solve has to report (limo_ctx_last_solve_info)."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = _solve_batch(ctx, ws)
    info = ctx.last_solve_info()
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    assert info["path"] == path and info["recovered"] == 0, (env, info)
    return out


def _streaming(ctx, monkeypatch):
    if "stream" not in _cache:
        _cache["stream"] = _solve(ctx, windows(), monkeypatch, STREAMING, "STREAMING")
    return _cache["stream"]


def _same(a, b, what):
    assert a[0] == b[0], (what, dict(zip(REPORT_KEYS, a[0])), dict(zip(REPORT_KEYS, b[0])))
    for name, x, y in zip(("kf_pose", "kf_plane_dir", "kf_plane_dist", "lm_pos", "trimmed"), a[1:], b[1:]):
        assert x == y, (what, name)
    assert np.isfinite(np.frombuffer(a[1])).all() and np.isfinite(np.frombuffer(a[4])).all(), what


def _label(i):
    return CASES[i][0]["name"] + "/" + CASES[i][1]


def test_windows_are_what_the_cases_are_for():
    ws = windows()
    for (s, v), w in zip(CASES, ws):
        assert (w.n_kf, w.n_lm, w.n_cam) == (s["n_kf"], s["n_lm"], 2 if "stereo_baseline" in s else 1)
        check_not_degenerate(w, v)
        if v == "sparse":
            assert sorted(set(w.obs_kf[w.obs_lm == 0])) == [0, 1]
            assert not ((w.obs_lm == w.n_lm - 1) & (views_of(w) == w.n_kf * w.n_cam - 1)).any() or w.n_kf == 2
    by = {s["name"]: w for (s, v), w in zip(CASES, ws) if v == "sparse"}
    assert not by["a"].lm_is_ground.any() and not by["b"].lm_is_ground.any() and not by["c"].lm_is_ground.any()
    assert by["b_ground"].lm_is_ground.all()


def test_every_window_matches_the_oracle(ctx, oracle, monkeypatch):
    got = _streaming(ctx, monkeypatch)
    trimmed = 0
    for i, w in enumerate(windows()):
        wo = w.copy()
        ro, _ = oracle.solve(wo, options())
        rep = dict(zip(REPORT_KEYS, got[i][0]))
        pose = np.frombuffer(got[i][1]).reshape(-1, 7)
        assert rep["n_trimmed_landmarks"] == ro["n_trimmed_landmarks"], _label(i)
        assert abs(rep["final_cost"] - ro["final_cost"]) <= TOL * abs(ro["final_cost"]), _label(i)
        assert np.abs(pose[:, 4:] - wo.kf_pose[:, 4:]).max() / max(1e-12, np.abs(wo.kf_pose[:, 4:]).max()) <= TOL, _label(i)
        assert np.array_equal(pose[0], w.kf_pose[0]), _label(i)  # keyframe 0 is Pose-fixed
        trimmed += rep["n_trimmed_landmarks"] > 0
    assert trimmed >= 1  # a trimming round that removes landmarks


def test_lock_step_equals_streaming(ctx, monkeypatch):
    got = _solve(ctx, windows(), monkeypatch, LOCK_STEP, "LOCKSTEP")
    ref = _streaming(ctx, monkeypatch)
    for i in range(len(CASES)):
        _same(ref[i], got[i], _label(i))


def test_one_launch_equals_streaming(ctx, monkeypatch):
    got = _solve(ctx, [windows()[i] for i in FAST], monkeypatch, {}, "COOP")
    ref = _streaming(ctx, monkeypatch)
    for k, i in enumerate(FAST):
        _same(ref[i], got[k], _label(i))


def test_streaming_under_poison_equals_streaming(ctx, monkeypatch):
    env = {k: v for k, v in os.environ.items() if k not in _ENV}
    env.update(STREAMING, KBA_POISON="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split()[1] for l in r.stdout.splitlines() if l.startswith("digest ")]
    assert lines == [_digest(x) for x in _streaming(ctx, monkeypatch)]
    assert [l.split()[1] for l in r.stdout.splitlines() if l.startswith("path ")] == ["STREAMING"]


if __name__ == "__main__":  # the streaming solve of all windows in a process of its own (KBA_POISON is read once per process)
    _ctx = ba.Context(0)
    for res in _solve_batch(_ctx, windows()):
        print("digest", _digest(res))
    print("path", _ctx.last_solve_info()["path"])
