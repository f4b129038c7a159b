"""Per-window solve options on the GPU: limo_ba_batch_solve_each / limo_ba_adjust_pose_only_batch_each (include/limo_hip.h).

The contract: window i of a batch solved with opts[i] gets the result of the single call made with opts[i], bit for bit - parameter
arrays, trimmed set, every integer of the report, both costs - on every launch path; an array of equal entries IS the one-options
call; what may not differ is refused before anything is launched.  The single calls are made once (module fixture) and shared.

Not covered here: the refusal of a landmark-sharded batch.  The library has it (limo_hip.hip:limo_ba_batch_solve_each), but no
entry point of the C-ABI hands a sharded batch to the caller - limo_ba_solve_sharded makes and destroys its own - so no test can
reach it.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import fuzz_common as fc
import lockstep_common as lc
import window_options_common as woc
from limo_amd import _ffi, ba, default_options, synth

pytestmark = pytest.mark.gpu

PATH_SWITCHES = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_COOP_MAX_WIN", "KBA_GROUPS", "KBA_COOP_TIMEOUT_MS")
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "num_linearizations",
               "n_depth_blocks", "n_repr_blocks", "n_gp_blocks", "n_trimmed_landmarks", "initial_cost", "final_cost")
POSE_REPORT_KEYS = ("final_cost", "initial_cost", "iterations_total", "iterations_final", "num_solves", "n_trimmed_landmarks", "termination",
                    "successful_steps", "num_linearizations")  # (tests/test_gpu_pose_batch.py)


def _force(monkeypatch, path):
    """The launch path of the next solves, the way tests/test_gpu_fixed_landmarks.py forces them (None: the library's own choice)."""
    for k in PATH_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if path in ("STREAMING", "LOCKSTEP"):
        monkeypatch.setenv("KBA_NO_COOP_SOLVE", "1")
        monkeypatch.setenv("KBA_NO_WG_SOLVE", "1")
        monkeypatch.setenv("KBA_STREAM_MIN", "1" if path == "STREAMING" else "100000")
    elif path == "COOP":
        monkeypatch.setenv("KBA_NO_WG_SOLVE", "1")


def _state(b, reps):
    return [(tuple(r[k] for k in REPORT_KEYS), w.kf_pose.copy(), w.kf_plane_dir.copy(), w.kf_plane_dist.copy(), w.lm_pos.copy(), b.trimmed(i))
            for i, (w, r) in enumerate(zip(b.windows, reps))]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], (what, i, dict(zip(REPORT_KEYS, x[0])), dict(zip(REPORT_KEYS, y[0])))
        assert all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:])), (what, i)


def _single(ctx, w, o, lm_fixed=None):
    """The single call, in its resident form (a batch of one: it can tell the trimmed set)."""
    b = ba.Batch(ctx, [w.copy()], lm_fixed=None if lm_fixed is None else [lm_fixed])
    b.solve(o)
    st = _state(b, b.download())[0]
    b.close()
    return st


@pytest.fixture(scope="module")
def singles(ctx):
    """Window i under its own options and - where they differ from entry 0's - under entry 0's, on the default path."""
    saved = {k: os.environ.pop(k) for k in PATH_SWITCHES if k in os.environ}
    try:
        ws, os_ = woc.windows(), woc.window_options()
        own = [_single(ctx, w, o) for w, o in zip(ws, os_)]
        # limo_ba_solve itself, for one window: the resident form of one window is the same call
        x = ws[3].copy()
        r = ctx.solve(x, os_[3])
        assert tuple(r[k] for k in REPORT_KEYS) == own[3][0] and np.array_equal(x.kf_pose, own[3][1]) and np.array_equal(x.lm_pos, own[3][4])
        under0 = {i: _single(ctx, ws[i], os_[0]) for i in range(len(ws)) if not woc.same_options(i)}
    finally:
        os.environ.update(saved)
    return own, under0


def test_the_inputs_can_tell(singles):
    """Every window whose options differ from entry 0's comes out differently under them, in trimmed set or final cost: a batch that
    gave every window entry 0's options could not pass the tests below."""
    own, under0 = singles
    assert len(under0) >= 8 and any(woc.same_options(i) for i in range(1, len(own)))
    for i, s0 in under0.items():
        assert (not np.array_equal(own[i][5], s0[5])) or own[i][0][-1] != s0[0][-1], i
    assert sum(1 for i, s0 in under0.items() if not np.array_equal(own[i][5], s0[5])) >= 3  # the quantiles decide somewhere


@pytest.mark.parametrize("path", ["STREAMING", "LOCKSTEP"])
def test_batch_equals_single_calls(ctx, singles, path, monkeypatch):
    own, _ = singles
    ws, os_ = woc.windows(), woc.window_options()
    _force(monkeypatch, path)
    b = ba.Batch(ctx, [w.copy() for w in ws])
    b.solve(os_)
    assert ctx.last_solve_info()["path"] == path
    _assert_same(_state(b, b.download()), own, path)
    b.reset()
    b.solve(os_)
    assert ctx.last_solve_info()["path"] == path
    _assert_same(_state(b, b.download()), own, path + " after reset")
    b.close()


def test_batch_equals_single_calls_coop(ctx, singles, monkeypatch):
    own, _ = singles
    ws, os_ = woc.windows(), woc.window_options()
    sub = woc.COOP_SUBSET
    assert len(sub) >= 8 and any(not woc.same_options(i, sub[0]) for i in sub)
    _force(monkeypatch, "COOP")
    b = ba.Batch(ctx, [ws[i].copy() for i in sub])
    b.solve([os_[i] for i in sub])
    info = ctx.last_solve_info()
    assert info["path"] == "COOP" and info["recovered"] == 0, info
    _assert_same(_state(b, b.download()), [own[i] for i in sub], "COOP")
    b.close()


def test_iteration_log_on(ctx, singles, monkeypatch):
    """With the iteration log switched on: the same results, and window i's log is the log of its single call."""
    own, _ = singles
    ws, os_ = woc.windows(), woc.window_options()
    sub = (1, 3, 5, 6)
    _force(monkeypatch, None)
    ctx.set_iteration_log(True)
    try:
        logs = []
        for i in sub:
            ctx.solve(ws[i].copy(), os_[i])
            logs.append(ctx.last_iteration_log(0))
        _force(monkeypatch, "LOCKSTEP")
        b = ba.Batch(ctx, [ws[i].copy() for i in sub])
        b.solve([os_[i] for i in sub])
        assert ctx.last_solve_info()["path"] == "LOCKSTEP"
        _assert_same(_state(b, b.download()), [own[i] for i in sub], "log on")
        for k, i in enumerate(sub):
            got = b.iteration_log(k)
            assert len(got) == len(logs[k]) > 0 and got.tobytes() == logs[k].tobytes(), i
        b.close()
    finally:
        ctx.set_iteration_log(False)


# ---------------------------------------------------------------------------------------------- pose-only
POSE_SEED0 = 71


def _pose_opts(i):
    d, r, qd, qr = woc.DRAWN[1 + i % (len(woc.DRAWN) - 1)] if i % 3 else woc.DRAWN[0]
    return default_options(min_landmarks_for_trimming=30, depth_thres=d, reprojection_thres=r, depth_quantile=qd, reprojection_quantile=qr)


_pose_single_cache = {}


def _pose_single(ctx, i):
    if i not in _pose_single_cache:
        pw, prior, _ = synth.make_pose_only_case(POSE_SEED0 + i)
        x = pw.copy()
        rep = ctx.adjust_pose_only(x, prior if i % 2 == 0 else None, _pose_opts(i))
        _pose_single_cache[i] = (x.kf_pose.tobytes(), rep)
    return _pose_single_cache[i]


@pytest.mark.parametrize("no_wg", [False, True])
@pytest.mark.parametrize("n", [2, 7, 65])
def test_pose_only_batch_equals_single_calls(ctx, n, no_wg, monkeypatch):
    _force(monkeypatch, None)
    refs = [_pose_single(ctx, i) for i in range(n)]
    if no_wg:
        monkeypatch.setenv("KBA_NO_WG_SOLVE", "1")
    cases = [synth.make_pose_only_case(POSE_SEED0 + i) for i in range(n)]
    wins = [c[0].copy() for c in cases]
    priors = [c[1] if i % 2 == 0 else None for i, c in enumerate(cases)]
    opts = [_pose_opts(i) for i in range(n)]
    assert any(o.depth_thres != opts[0].depth_thres for o in opts) and any(o.depth_quantile != opts[0].depth_quantile for o in opts)
    reps = ctx.adjust_pose_only_batch(wins, priors, opts)
    assert ctx.last_solve_info()["path"] == ("LOCKSTEP" if no_wg else "WG")
    for i in range(n):
        assert wins[i].kf_pose.tobytes() == refs[i][0], i
        for k in POSE_REPORT_KEYS:
            assert reps[i][k] == refs[i][1][k], (i, k, reps[i][k], refs[i][1][k])
    assert any(r["n_trimmed_landmarks"] > 0 for r in reps)
    assert len({(r["n_trimmed_landmarks"], r["final_cost"]) for r in reps}) > 1


# ---------------------------------------------------------------------------------------------- uniform and back
def test_uniform_list_is_the_one_options_call_and_back(ctx, singles, monkeypatch):
    own, _ = singles
    ws, os_ = woc.windows(), woc.window_options()
    o = os_[0]
    _force(monkeypatch, "LOCKSTEP")
    b = ba.Batch(ctx, [w.copy() for w in ws])
    b.solve(o)
    uniform = _state(b, b.download())
    b.reset()
    b.solve([default_options() for _ in ws])  # equal entries (copies): the path of solve(o)
    _assert_same(_state(b, b.download()), uniform, "list of equal options")
    b.reset()
    b.solve(os_)
    _assert_same(_state(b, b.download()), own, "differing list")
    b.reset()
    b.solve(o)  # uniform again: no table left in any view
    _assert_same(_state(b, b.download()), uniform, "uniform after a differing list")
    b.close()
    _force(monkeypatch, "STREAMING")  # (the slot groups keep views of their own)
    b = ba.Batch(ctx, [w.copy() for w in ws])
    b.solve(os_)
    _assert_same(_state(b, b.download()), own, "streaming, differing list")
    b.reset()
    b.solve(o)
    _assert_same(_state(b, b.download()), uniform, "streaming, uniform after a differing list")
    b.close()


def test_fixed_landmark_batch_equals_its_single_calls(ctx, monkeypatch):
    ws, os_ = woc.windows(), woc.window_options()
    sub = (2, 3, 5, 7)
    rng = np.random.default_rng(5)
    flags = [(rng.random(ws[i].n_lm) < 0.4).astype(np.uint8) for i in sub]
    _force(monkeypatch, None)
    want = [_single(ctx, ws[i], os_[i], lm_fixed=f) for i, f in zip(sub, flags)]
    for path in ("LOCKSTEP", "STREAMING"):
        _force(monkeypatch, path)
        b = ba.Batch(ctx, [ws[i].copy() for i in sub], lm_fixed=flags)
        b.solve([os_[i] for i in sub])
        assert ctx.last_solve_info()["path"] == path
        _assert_same(_state(b, b.download()), want, "fixed landmarks, " + path)
        b.close()


# ---------------------------------------------------------------------------------------------- against the oracle
def test_differing_list_matches_the_oracle(ctx, oracle, monkeypatch):
    """Three windows with non-default thresholds, solved as one batch with their own options, held to fuzz_common.check_parity
    against pyoracle.solve(w, opts[i]): identical trimmed sets, 1e-4 on cost and keyframe translations, never the iteration-cap clause."""
    ws, os_ = woc.windows(), woc.window_options()
    sub = (2, 3, 5)
    assert all(os_[i].depth_thres != 0.16 or os_[i].reprojection_thres != 1.6 for i in sub)
    _force(monkeypatch, "LOCKSTEP")
    b = ba.Batch(ctx, [ws[i].copy() for i in sub])
    b.solve([os_[i] for i in sub])
    reps = b.download()
    _force(monkeypatch, None)
    for k, i in enumerate(sub):
        o = os_[i]
        wo = ws[i].copy()
        ro, _ = oracle.solve(wo, o)
        to = oracle.last_trimmed()
        tg = b.trimmed(k)
        so = lambda p, _o, o=o: oracle.solve(p, o)[0]  # (the sensitivity re-runs use the window's own options)
        sg = lambda p, _o, o=o: ctx.solve(p, o)
        ok, detail, clause = fc.check_parity(ws[i], reps[k], b.windows[k], tg, sg, ro, wo, to, so)
        print("window %d: %s; final cost %.9g / %.9g" % (i, detail, reps[k]["final_cost"], ro["final_cost"]))
        assert ok, (i, detail)
        assert clause != fc.BY_CAP
    b.close()


# ---------------------------------------------------------------------------------------------- refusals
def _err(ctx):
    return ctx.lib.limo_last_error(ctx.ptr).decode()


def test_refusals_launch_nothing(ctx, singles, monkeypatch):
    own, _ = singles
    ws, os_ = woc.windows(), woc.window_options()
    sub = (0, 2, 3, 5)
    _force(monkeypatch, "LOCKSTEP")
    b = ba.Batch(ctx, [ws[i].copy() for i in sub])
    lib = ctx.lib

    def call(opts):
        arr, n = ba.options_array(opts)
        return lib.limo_ba_batch_solve_each(b.ptr, n, arr)

    good = [os_[i] for i in sub]
    assert call(good[:3]) == _ffi.LIMO_ERR_INVALID and "n_opts" in _err(ctx)
    bad = [woc.options(woc.DRAWN[i]) for i in sub]
    bad[3].max_num_iterations = 50
    assert call(bad) == _ffi.LIMO_ERR_INVALID and "window 3: max_num_iterations" in _err(ctx)
    bad = [woc.options(woc.DRAWN[i]) for i in sub]
    bad[2].min_landmarks_for_trimming = 30
    assert call(bad) == _ffi.LIMO_ERR_INVALID and "window 2: min_landmarks_for_trimming" in _err(ctx)
    for value in (math.nan, math.inf):
        bad = [woc.options(woc.DRAWN[i]) for i in sub]
        bad[1].depth_thres = value
        assert call(bad) == _ffi.LIMO_ERR_INVALID and "window 1: depth_thres" in _err(ctx)
    assert lib.limo_ba_batch_solve_each(b.ptr, len(sub), None) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_ba_batch_solve_each(None, len(sub), ba.options_array(good)[0]) == _ffi.LIMO_ERR_INVALID
    # nothing was launched: the batch is in its created state and solves normally
    reps = b.download()
    assert all(r["num_solves"] == 0 and r["iterations_total"] == 0 for r in reps)
    assert all(np.array_equal(x.kf_pose, ws[i].kf_pose) and np.array_equal(x.lm_pos, ws[i].lm_pos) for x, i in zip(b.windows, sub))
    b.solve(good)
    _assert_same(_state(b, b.download()), [own[i] for i in sub], "after the refusals")
    b.close()
    # the pose-only form
    cases = [synth.make_pose_only_case(POSE_SEED0 + i) for i in range(3)]
    wins = [c[0].copy() for c in cases]
    from limo_amd.window import struct_array

    arr = struct_array(wins)
    opts = [_pose_opts(i) for i in range(3)]
    opts[2].trim_solver_iterations = 5
    oarr, _ = ba.options_array(opts)
    reps = (_ffi.BaReport * 3)()
    assert lib.limo_ba_adjust_pose_only_batch_each(ctx.ptr, 3, arr, None, oarr, reps) == _ffi.LIMO_ERR_INVALID
    assert "window 2: trim_solver_iterations" in _err(ctx)
    assert lib.limo_ba_adjust_pose_only_batch_each(ctx.ptr, 3, arr, None, None, reps) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_ba_adjust_pose_only_batch_each(ctx.ptr, 3, None, None, oarr, reps) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_ba_adjust_pose_only_batch_each(None, 3, arr, None, oarr, reps) == _ffi.LIMO_ERR_INVALID
    assert all(np.array_equal(w.kf_pose, c[0].kf_pose) for w, c in zip(wins, cases))
    with pytest.raises(ValueError):
        ctx.adjust_pose_only_batch(wins, None, opts[:2])


# ---------------------------------------------------------------------------------------------- the drive
SWEEP_LINES = (
    "depth_thres=0.08 reprojection_thres=3.0 outlier_quantile=0.8 shrubbery_weight=0.5",
    "depth_thres=0.4 reprojection_thres=0.8 outlier_quantile=0.9 shrubbery_weight=0.9",
    "depth_thres=0.16 reprojection_thres=1.6 outlier_quantile=0.95 shrubbery_weight=0.7",
    "depth_thres=0.3 reprojection_thres=2.4 outlier_quantile=0.85 shrubbery_weight=1.0",
)


def _flags(line):
    kv = dict(t.split("=") for t in line.split())
    return ["--depth-thres", kv["depth_thres"], "--reprojection-thres", kv["reprojection_thres"], "--outlier-quantile", kv["outlier_quantile"],
            "--shrubbery-weight", kv["shrubbery_weight"]]


def test_sweep_drive_equals_the_single_drives(tmp_path):
    """apps/limo_stream on liblimo_hip.so, four sequences over ONE world (seed 7) with a parameter set each: sequence i's pose file
    is the single drive with that line's flags, byte for byte, and the pose-only and solve stages made batched calls that carried
    differing options (limo_ba_adjust_pose_only_batch_each / limo_ba_batch_solve_each)."""
    import emu_ffi

    exe = emu_ffi.build_stream_app(gpu=True)
    sweep = tmp_path / "sweep.txt"
    sweep.write_text("\n".join(SWEEP_LINES) + "\n")
    info, files = lc.run_lockstep(exe, ["--sequences", "4", "--frames", "60", "--az", "2000", "--seed", "7", "--sweep", str(sweep)], str(tmp_path / "sweep_poses"),
                                  timeout=300)
    print(json.dumps(info))
    for st in ("pose_only", "solve"):
        s = info["stages"][st]
        assert s["fallback_calls"] == 0 and s["max_items"] > 1 and s["per_window_calls"] > 0, (st, s)
    for i, l in enumerate(SWEEP_LINES):
        want, _ = lc.single_rows(exe, 60, 7, ["--az", "2000"] + _flags(l), tmp_path, timeout=300)
        assert files[i] == want, "sequence %d" % i
    assert len(set(files)) >= 2
