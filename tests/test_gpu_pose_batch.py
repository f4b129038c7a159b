"""The batched pose-only adjustment on the GPU: limo_ba_adjust_pose_only_batch / limo_ba_batch_create_pose_only.

The contract (include/limo_hip.h): window i of a batch gets the result of limo_ba_adjust_pose_only(window i, prior i) bit for bit -
pose, every integer of the report, initial_cost and final_cost - on both launch paths a batch of several windows can take (one
k_solve_wg launch with a workgroup per window; the lock-step launch sequence).  The single calls are made once per (seed, prior, cap)
and shared by the tests.
"""
import functools

import numpy as np
import pytest

from limo_amd import _ffi, ba, default_options, synth
from limo_amd.window import Window

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_ba.py: north_star tolerance on the final cost
_ENV = ("KBA_NO_WG_SOLVE", "KBA_NO_COOP_SOLVE", "KBA_STREAM_MIN", "KBA_COOP_MAX_WIN")
REPORT_KEYS = ("final_cost", "initial_cost", "iterations_total", "iterations_final", "num_solves", "n_trimmed_landmarks", "termination",
               "successful_steps", "num_linearizations")  # (the fields test_pose_only_one_launch_equals_lock_step lists)
SEED0 = 71


@functools.lru_cache(maxsize=None)
def _case(seed):
    pw, prior, _ = synth.make_pose_only_case(seed)
    return pw, prior


def _opts(cap=-1.0):
    return default_options(min_landmarks_for_trimming=30, max_solver_time_sec=cap)


def _clear_env(monkeypatch):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)


_single_cache = {}


def _single(ctx, monkeypatch, seed, with_prior, cap):
    """limo_ba_adjust_pose_only of one case on the default path: (pose bytes, report), computed once."""
    key = (seed, bool(with_prior), cap)
    if key not in _single_cache:
        _clear_env(monkeypatch)
        pw, prior = _case(seed)
        x = pw.copy()
        rep = ctx.adjust_pose_only(x, prior if with_prior else None, _opts(cap))
        assert np.array_equal(x.lm_pos, pw.lm_pos)
        _single_cache[key] = (x.kf_pose.tobytes(), rep)
    return _single_cache[key]


def _batch_inputs(n):
    """n windows of seeds 71.., a prior on every second one."""
    wins = [_case(SEED0 + i)[0].copy() for i in range(n)]
    priors = [_case(SEED0 + i)[1] if i % 2 == 0 else None for i in range(n)]
    return wins, priors


def _assert_same(pose_bytes, rep, ref, what):
    assert pose_bytes == ref[0], what
    for k in REPORT_KEYS:
        assert rep[k] == ref[1][k], (what, k, rep[k], ref[1][k])


def _check_against_singles(ctx, monkeypatch, wins, reps, cap):
    for i, (w, r) in enumerate(zip(wins, reps)):
        _assert_same(w.kf_pose.tobytes(), r, _single(ctx, monkeypatch, SEED0 + i, i % 2 == 0, cap), "window %d" % i)
        assert np.array_equal(w.lm_pos, _case(SEED0 + i)[0].lm_pos)  # landmarks are constant
    assert any(r["n_trimmed_landmarks"] > 0 and r["num_solves"] >= 2 for r in reps)  # the trimming branch ran


@pytest.mark.parametrize("cap", [-1.0, 20.0])
@pytest.mark.parametrize("n", [1, 2, 7, 65, 300])
def test_batch_equals_single_calls(ctx, n, cap, monkeypatch):
    """65 windows: past the 64-window limit of the one-launch paths of other batches; 300: more workgroups than the chip has CUs."""
    refs = [_single(ctx, monkeypatch, SEED0 + i, i % 2 == 0, cap) for i in range(n)]  # (before the batch: the same default path)
    assert len(refs) == n
    _clear_env(monkeypatch)
    wins, priors = _batch_inputs(n)
    reps = ctx.adjust_pose_only_batch(wins, priors, _opts(cap))
    assert ctx.last_solve_info()["path"] == "WG"  # one launch at every size, with and without the cap
    assert len(reps) == n
    _check_against_singles(ctx, monkeypatch, wins, reps, cap)
    assert len({r["time_sec"] for r in reps}) == 1  # the batch's time


@pytest.mark.parametrize("n", [7, 65])
def test_both_launch_paths(ctx, n, monkeypatch):
    """One k_solve_wg launch and the lock-step sequence (KBA_NO_WG_SOLVE=1): identical to each other and to the single calls.  The
    resident batch tells which path ran: only the lock-step sequence times its linearisation launches."""
    refs = [_single(ctx, monkeypatch, SEED0 + i, i % 2 == 0, -1.0) for i in range(n)]
    assert len(refs) == n
    runs = []
    for env in ({}, {"KBA_NO_WG_SOLVE": "1"}):
        _clear_env(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        wins, priors = _batch_inputs(n)
        reps = ctx.adjust_pose_only_batch(wins, priors, _opts())
        assert ctx.last_solve_info()["path"] == ("LOCKSTEP" if env else "WG")
        b = ba.Batch(ctx, _batch_inputs(n)[0], pose_only=True, priors=priors)
        b.solve(_opts())
        assert ctx.last_solve_info()["path"] == ("LOCKSTEP" if env else "WG")
        launches = b.kernel_stats()["linearize_launches"]
        b.close()
        _clear_env(monkeypatch)
        assert (launches > 0) == bool(env), (env, launches)
        _check_against_singles(ctx, monkeypatch, wins, reps, -1.0)
        runs.append((wins, reps))
    (wa, ra), (wb, rb) = runs
    for i in range(n):
        _assert_same(wb[i].kf_pose.tobytes(), rb[i], (wa[i].kf_pose.tobytes(), ra[i]), "window %d, lock-step against one launch" % i)


def _pose_only_of(w, keep_lm=None):
    """The newest keyframe of window w against its landmarks at their ground-truth positions, and the speed prior from the two
    keyframes before it: limo_amd/synth.py:make_pose_only_case for any window; keep_lm: only the first keep_lm landmarks."""
    k = w.n_kf - 1
    n_lm = w.n_lm if keep_lm is None else keep_lm
    sel = (w.obs_kf == k) & (w.obs_lm < n_lm)
    pw = Window(kf_pose=w.kf_pose[k:k + 1].copy(), kf_plane_dir=w.kf_plane_dir[k:k + 1], kf_plane_dist=w.kf_plane_dist[k:k + 1],
                kf_fixation=np.array([_ffi.LIMO_FIX_NONE], np.int32), cam=w.cam, lm_pos=w.meta["gt_lm"][:n_lm].copy(), lm_weight=w.lm_weight[:n_lm],
                lm_is_ground=w.lm_is_ground[:n_lm], obs_kf=np.zeros(sel.sum(), np.int32), obs_lm=w.obs_lm[sel], obs_cam=w.obs_cam[sel],
                obs_u=w.obs_u[sel], obs_v=w.obs_v[sel], obs_d=w.obs_d[sel])
    prior = _ffi.SpeedPrior()
    prior.speed_weight = 0.7
    prior.dt_cur = 0.4
    pb = w.meta["gt_pose"][k - 1]
    prior.pose_before[:] = pb.tolist()
    Rb, tb = synth.pose_to_Rt(pb)
    Rbb, tbb = synth.pose_to_Rt(w.meta["gt_pose"][k - 2])
    prior.vel_prev[:] = ((tb - Rb @ Rbb.T @ tbb) / 0.4).tolist()
    return pw, prior


def test_ragged_batch_takes_the_lock_step_sequence(ctx, monkeypatch):
    """A 300-landmark window, the same window cut down to 20 landmarks (<= 30: it does not trim, one solve) and a window made from
    make_window(n_kf=4, n_lm=2200) (more than 2048 landmarks: nine landmark workgroups, more than k_solve_wg walks through): the
    whole batch takes the lock-step sequence, and every window still gets its single call's bits."""
    _clear_env(monkeypatch)
    base = synth.make_window(SEED0, n_kf=4, n_lm=300, outlier_frac=0.02)
    full, prior = _pose_only_of(base)
    assert full.kf_pose.tobytes() == _case(SEED0)[0].kf_pose.tobytes() and np.array_equal(full.obs_u, _case(SEED0)[0].obs_u)  # make_pose_only_case(71)
    small, _ = _pose_only_of(base, keep_lm=20)
    big, prior_big = _pose_only_of(synth.make_window(SEED0 + 1, n_kf=4, n_lm=2200, outlier_frac=0.02))
    assert small.n_lm == 20 and big.n_lm > 2048  # (make_window keeps the landmarks some keyframe sees: a few less than it is asked for)
    wins0, priors = [full, small, big], [prior, None, prior_big]
    o = _opts()
    singles = []
    for w, p in zip(wins0, priors):
        x = w.copy()
        rep = ctx.adjust_pose_only(x, p, o)
        singles.append((x.kf_pose.tobytes(), rep))
    wins = [w.copy() for w in wins0]
    reps = ctx.adjust_pose_only_batch(wins, priors, o)
    assert ctx.last_solve_info()["path"] == "LOCKSTEP"
    for i in range(3):
        _assert_same(wins[i].kf_pose.tobytes(), reps[i], singles[i], "window %d" % i)
        assert np.array_equal(wins[i].lm_pos, wins0[i].lm_pos)
    assert reps[1]["num_solves"] == 1 and reps[1]["n_trimmed_landmarks"] == 0
    assert reps[0]["num_solves"] >= 2 and reps[0]["n_trimmed_landmarks"] > 0
    assert reps[2]["num_solves"] >= 2
    b = ba.Batch(ctx, [w.copy() for w in wins0], pose_only=True, priors=priors)
    b.solve(o)
    assert ctx.last_solve_info()["path"] == "LOCKSTEP"
    assert b.kernel_stats()["linearize_launches"] > 0  # launches of k_lin_lm: the lock-step sequence, not k_solve_wg
    reps2 = b.download()
    for i in range(3):
        _assert_same(b.windows[i].kf_pose.tobytes(), reps2[i], singles[i], "resident window %d" % i)
    b.close()


def test_resident_form(ctx, monkeypatch):
    n = 7
    refs = [_single(ctx, monkeypatch, SEED0 + i, i % 2 == 0, -1.0) for i in range(n)]
    _clear_env(monkeypatch)
    o = _opts()
    wins, priors = _batch_inputs(n)
    b = ba.Batch(ctx, wins, pose_only=True, priors=priors)
    b.solve(o)
    assert b.kernel_stats()["linearize_launches"] == 0  # one k_solve_wg launch
    assert ctx.last_solve_info()["path"] == "WG"
    r1 = b.download()
    p1 = [w.kf_pose.tobytes() for w in b.windows]
    b.reset()
    b.solve(o)
    assert ctx.last_solve_info()["path"] == "WG"
    r2 = b.download()
    p2 = [w.kf_pose.tobytes() for w in b.windows]
    one_shot_w, _ = _batch_inputs(n)
    one_shot_r = ctx.adjust_pose_only_batch(one_shot_w, priors, o)
    for i in range(n):
        _assert_same(p1[i], r1[i], refs[i], "first solve, window %d" % i)
        _assert_same(p2[i], r2[i], refs[i], "solve after reset, window %d" % i)
        _assert_same(one_shot_w[i].kf_pose.tobytes(), one_shot_r[i], refs[i], "one-shot call, window %d" % i)
        assert np.array_equal(b.windows[i].lm_pos, _case(SEED0 + i)[0].lm_pos)
    any_trimmed = False
    for i in range(n):  # the trimmed set of the single call's path: a pose-only batch of that one window
        s = ba.Batch(ctx, [_case(SEED0 + i)[0].copy()], pose_only=True, priors=[priors[i]])
        s.solve(o)
        want = s.trimmed(0)
        assert s.download()[0]["n_trimmed_landmarks"] == len(want) == refs[i][1]["n_trimmed_landmarks"]
        s.close()
        got = b.trimmed(i)
        assert np.array_equal(got, want), i
        any_trimmed = any_trimmed or len(got) > 0
    assert any_trimmed
    b.close()


@pytest.mark.parametrize("with_prior", [False, True])
def test_batch_matches_oracle(ctx, oracle, with_prior, monkeypatch):
    """Seeds 71-74 against the oracle at the bars of test_pose_only_matches_oracle."""
    _clear_env(monkeypatch)
    seeds = [71, 72, 73, 74]
    o = _opts()
    wins = [_case(s)[0].copy() for s in seeds]
    priors = [_case(s)[1] for s in seeds] if with_prior else None
    reps = ctx.adjust_pose_only_batch(wins, priors, o)
    for i, s in enumerate(seeds):
        po = _case(s)[0].copy()
        ro = oracle.adjust_pose_only(po, _case(s)[1] if with_prior else None, o)
        print("seed %d prior %d: trimmed %d / %d, final cost %.12e / %.12e, max pose diff %.3e" % (
            s, with_prior, reps[i]["n_trimmed_landmarks"], ro["n_trimmed_landmarks"], reps[i]["final_cost"], ro["final_cost"],
            np.abs(wins[i].kf_pose - po.kf_pose).max()))
    for i, s in enumerate(seeds):
        po = _case(s)[0].copy()
        ro = oracle.adjust_pose_only(po, _case(s)[1] if with_prior else None, o)
        assert reps[i]["n_trimmed_landmarks"] == ro["n_trimmed_landmarks"], s
        assert abs(reps[i]["final_cost"] - ro["final_cost"]) <= TOL * abs(ro["final_cost"]), s
        assert np.abs(wins[i].kf_pose - po.kf_pose).max() <= 1e-6, s
        assert np.array_equal(wins[i].lm_pos, _case(s)[0].lm_pos)


def test_invalid_window_fails_the_batch_and_names_it(ctx, monkeypatch):
    _clear_env(monkeypatch)
    o = _opts()
    wins, priors = _batch_inputs(5)
    wins[3] = synth.make_window(5, n_kf=2, n_lm=40)
    before = [w.kf_pose.tobytes() for w in wins]
    with pytest.raises(ba.LimoError) as e:
        ctx.adjust_pose_only_batch(wins, priors, o)
    assert "window 3" in str(e.value) and "rc=%d" % _ffi.LIMO_ERR_INVALID in str(e.value)
    assert [w.kf_pose.tobytes() for w in wins] == before  # nothing was solved
    with pytest.raises(ba.LimoError) as e:
        ba.Batch(ctx, wins, pose_only=True, priors=priors)
    assert "window 3" in str(e.value)
    with pytest.raises(ba.LimoError):
        ctx.adjust_pose_only_batch([], None, o)
    # the context is as good as before
    wins, priors = _batch_inputs(5)
    reps = ctx.adjust_pose_only_batch(wins, priors, o)
    _check_against_singles(ctx, monkeypatch, wins, reps, -1.0)
