"""One LM step on the GPU against the dense reference of tests/lm_step_common.py for the solve paths that run device code of their
own and were held to the oracle only at 1e-4 after tens of iterations, or to each other bit for bit:

  * fixed-landmark windows (limo_ba_batch_create_fixed_landmarks, limo_ba_solve_fixed_landmarks): the constant run of the packed
    landmarks, the fixed-cost slot of the camera assembly, Schur worklists without the constant landmarks, views without a free pose
    block - the shapes of fixed_lm_common.shapes(), one resident batch per option set;
  * the pose-only adjustment (limo_ba_batch_create_pose_only, limo_ba_adjust_pose_only): the speed-prior rows, landmark state 2, the
    6-column system without Schur blocks, k_solve_wg and the lock-step sequence - make_pose_only_case(71..74) with the prior, without
    one, with speed_weight = 0, and a window cut down to 20 landmarks;
  * the landmark-sharded solve (limo_ba_solve_sharded): k_shard_reduce, k_slab_reduce, k_unpack and the two-piece exchange of the
    first iteration, over few and many virtual shards, down to shards without a landmark, and once over a one-rank RCCL communicator.
    It records no iteration log: parameters and report only (lm_step_common.check_params_only).

Every window goes through check_step / check_params_only at lm_step_common.BARS, which the CPU tier sets
(tests/test_lm_step_cpu.py).  The GPU's own deviation per class is printed by every test (pytest -s) before it is held to the bars
and recorded in profiles/lm_step_reference.md."""
import pytest

import lm_step_common as lsc
import test_gpu_lm_step as glm
from limo_amd import ba

pytestmark = pytest.mark.gpu

_ENV = glm._ENV
_LOCK = {"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}
FIXED_PATHS = {"default": {}, "LOCKSTEP": dict(_LOCK, KBA_STREAM_MIN="100000"), "STREAMING": dict(_LOCK, KBA_STREAM_MIN="1")}
POSE_PATHS = {"default": {}, "LOCKSTEP": {"KBA_NO_WG_SOLVE": "1"}}  # (default: one k_solve_wg launch, a workgroup per window)
REPORT_KEYS = glm.REPORT_KEYS
FIXED_CASES, POSE_CASES, SHARDED_CASES = lsc.fixed_cases(), lsc.pose_cases(), lsc.sharded_cases()
# the fixed-landmark batches that also run the other two launch paths: the default set, and windows (a) and (e_all) alone (a batch of
# one window; (e_all) has no variable landmark and so no Schur launch at all)
FIXED_PATH_BATCHES = {"default": None, "a": ("a",), "e_all": ("e_all",)}
POSE_PATH_CASES = ("default", "min_relative_decrease_10")

_cache = {}  # the batches' results: computed once, shared, never changed


def _set_path(monkeypatch, env):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _solve(ctx, windows, problems, o):
    """One resident batch of `windows` (all pose-only, or all solve windows with their flags) under `o`: [(after, report, log)] and
    what the solve launched."""
    if problems[0].pose_only:
        b = ba.Batch(ctx, [w.copy() for w in windows], pose_only=True, priors=[p.prior for p in problems])
    else:
        b = ba.Batch(ctx, [w.copy() for w in windows], lm_fixed=[p.lm_fixed for p in problems])
    try:
        b.solve(o)
        reps = b.download()
        return [(b.windows[i], reps[i], b.iteration_log(i)) for i in range(len(windows))], ctx.last_solve_info()
    finally:
        b.close()


def _runs(ctx, monkeypatch, kind, name, path, only=None):
    """window name -> (before, after, report, log, mid, problem) of the batch of a case of a problem kind on a launch path (mid: the
    batch's result after ONE iteration where the case takes two).  only: the windows of the batch (default: all of the case)."""
    key = (kind, name, path, only)
    if key not in _cache:
        cases, getw, paths = (FIXED_CASES, lsc.fixed_window, FIXED_PATHS) if kind == "fixed" else (POSE_CASES, lsc.pose_window, POSE_PATHS)
        names = [n for c, n in cases if c == name and (only is None or n in only)]
        assert names and (only is None or len(names) == len(only))
        pairs = [getw(n) for n in names]
        windows, problems = [w for w, _ in pairs], [p for _, p in pairs]
        o = lsc.case_options(name)
        _set_path(monkeypatch, paths[path])
        with glm._iteration_log(ctx):
            out, info = _solve(ctx, windows, problems, o)
            mids = _solve(ctx, windows, problems, lsc.one_step_options(o))[0] if o.max_num_iterations == 2 else [(None,)] * len(names)
        _set_path(monkeypatch, {})
        assert info["recovered"] == 0 and (path == "default" or info["path"] == path), (kind, name, path, info)
        _cache[key] = {n: (w,) + r + (m[0], p) for n, w, r, m, p in zip(names, windows, out, mids, problems)}
    return _cache[key]


def _hold(what, dev):
    print("GPU deviation", what, {c: "%.2e" % v for c, v in sorted(dev.items())})  # (printed before it is held to the bars)
    for cls, v in dev.items():
        assert v <= lsc.BARS[cls], (what, cls, "%.3e > %.1e" % (v, lsc.BARS[cls]))


def _assert_same_runs(want, got, what):
    assert list(got) == list(want)
    for n in want:
        for a, b in ((want[n][1], got[n][1]), (want[n][4], got[n][4])):
            assert (a is None and b is None) or lsc.same_bytes(a, b), (what, n)
        assert [got[n][2][k] for k in REPORT_KEYS] == [want[n][2][k] for k in REPORT_KEYS], (what, n)
        assert len(got[n][3]) == len(want[n][3]) and got[n][3].tobytes() == want[n][3].tobytes(), (what, n)


# ------------------------------------------------------------------------------------------------ fixed-landmark windows
@pytest.mark.parametrize("name,window", FIXED_CASES, ids=["%s-%s" % c for c in FIXED_CASES])
def test_fixed_landmark_step_against_the_dense_reference(ctx, monkeypatch, name, window):
    before, after, rep, log, mid, problem = _runs(ctx, monkeypatch, "fixed", name, "default")[window]
    dev = lsc.check_step(before, after, rep, log, lsc.case_options(name), mid=mid, bars=None, where="GPU fixed %s %s" % (name, window), problem=problem)
    _hold("fixed %s %s" % (name, window), dev)


@pytest.mark.parametrize("path", ["LOCKSTEP", "STREAMING"])
@pytest.mark.parametrize("batch", list(FIXED_PATH_BATCHES))
def test_fixed_landmark_step_same_bytes_on_every_launch_path(ctx, monkeypatch, batch, path):
    only = FIXED_PATH_BATCHES[batch]
    want = _runs(ctx, monkeypatch, "fixed", "default", "default", only)
    _assert_same_runs(want, _runs(ctx, monkeypatch, "fixed", "default", path, only), (batch, path))
    if only is not None:  # the window alone gets the bits it gets in the batch of all shapes
        whole = _runs(ctx, monkeypatch, "fixed", "default", "default")
        _assert_same_runs(want, {n: whole[n] for n in only}, (batch, "in the whole batch"))


def test_fixed_landmark_single_call_equals_the_batch(ctx, monkeypatch):
    """limo_ba_solve_fixed_landmarks and limo_ctx_last_iteration_log: the bytes of the window's entry in the resident batch."""
    _set_path(monkeypatch, {})
    for name, window in (("default", "h_b_02"), ("two_steps", "b")):
        before, after, rep, log, _, problem = _runs(ctx, monkeypatch, "fixed", name, "default")[window]
        x = before.copy()
        with glm._iteration_log(ctx):
            r = ctx.solve(x, lsc.case_options(name), problem.lm_fixed)
            single_log = ctx.last_iteration_log()
        assert lsc.same_bytes(x, after) and [r[k] for k in REPORT_KEYS] == [rep[k] for k in REPORT_KEYS], (name, window)
        assert len(single_log) == len(log) and single_log.tobytes() == log.tobytes(), (name, window)


def test_fixed_landmark_window_with_nothing_to_optimise(ctx, monkeypatch):
    """Shape (f): every block constant.  LIMO_CONVERGENCE, zero iterations, no log entry, the parameters bit for bit and
    initial_cost == final_cost == the problem's cost - from the batch and from the single call."""
    _set_path(monkeypatch, {})
    w, problem = lsc.fixed_window("f")
    o = lsc.case_options("default")
    with glm._iteration_log(ctx):
        (after, rep, log), = _solve(ctx, [w], [problem], o)[0]
        x = w.copy()
        r = ctx.solve(x, o, problem.lm_fixed)
        single_log = ctx.last_iteration_log()
    dev = lsc.check_nothing_to_optimise(w, after, rep, log, o, problem, bars=None, where="GPU f")
    _hold("fixed nothing to optimise", {"scalar": dev})
    assert lsc.same_bytes(x, after) and [r[k] for k in REPORT_KEYS] == [rep[k] for k in REPORT_KEYS] and len(single_log) == 0


# ------------------------------------------------------------------------------------------------ pose-only windows
@pytest.mark.parametrize("name,window", POSE_CASES, ids=["%s-%s" % c for c in POSE_CASES])
def test_pose_only_step_against_the_dense_reference(ctx, monkeypatch, name, window):
    runs = _runs(ctx, monkeypatch, "pose_only", name, "default")
    before, after, rep, log, mid, problem = runs[window]
    if window.endswith("_w0"):  # speed_weight = 0 is no prior: the bits of the window without one
        _assert_same_runs({window: runs[window[:-3] + "_none"][:5]}, {window: runs[window][:5]}, (name, "speed_weight = 0"))
    dev = lsc.check_step(before, after, rep, log, lsc.case_options(name), mid=mid, bars=None, where="GPU pose_only %s %s" % (name, window), problem=problem)
    _hold("pose_only %s %s" % (name, window), dev)


@pytest.mark.parametrize("name", POSE_PATH_CASES)
def test_pose_only_step_same_bytes_on_every_launch_path(ctx, monkeypatch, name):
    want = _runs(ctx, monkeypatch, "pose_only", name, "default")
    _assert_same_runs(want, _runs(ctx, monkeypatch, "pose_only", name, "LOCKSTEP"), (name, "KBA_NO_WG_SOLVE=1"))


def test_pose_only_single_call_equals_the_batch(ctx, monkeypatch):
    """limo_ba_adjust_pose_only and limo_ctx_last_iteration_log: the bytes of the window's entry in the resident batch."""
    _set_path(monkeypatch, {})
    for name, window in (("default", "72"), ("two_steps", lsc.POSE_SMALL)):
        before, after, rep, log, _, problem = _runs(ctx, monkeypatch, "pose_only", name, "default")[window]
        x = before.copy()
        with glm._iteration_log(ctx):
            r = ctx.adjust_pose_only(x, problem.prior, lsc.case_options(name))
            single_log = ctx.last_iteration_log()
        assert lsc.same_bytes(x, after) and [r[k] for k in REPORT_KEYS] == [rep[k] for k in REPORT_KEYS], (name, window)
        assert len(single_log) == len(log) and single_log.tobytes() == log.tobytes(), (name, window)


# ------------------------------------------------------------------------------------------------ the landmark-sharded solve
def _sharded(c, w, o, n_shards):
    """limo_ba_solve_sharded with the log switch ON: (after, report, what limo_ctx_last_iteration_log gives after it)."""
    after = w.copy()
    with glm._iteration_log(c):
        rep = c.solve_sharded(after, o, n_shards)
        log = c.last_iteration_log()
    return after, rep, log


def _sharded_run(ctx, monkeypatch, name, window, n_shards):
    key = ("sharded", name, window, n_shards)
    if key not in _cache:
        _set_path(monkeypatch, {})
        w, o = lsc.sharded_window(window), lsc.case_options(name)
        mid = _sharded(ctx, w, lsc.one_step_options(o), n_shards)[0] if o.max_num_iterations == 2 else None
        _cache[key] = (w,) + _sharded(ctx, w, o, n_shards) + (mid,)
    return _cache[key]


@pytest.mark.parametrize("name,window,n_shards", SHARDED_CASES, ids=["%s-%s-%d" % c for c in SHARDED_CASES])
def test_sharded_step_against_the_dense_reference(ctx, monkeypatch, name, window, n_shards):
    before, after, rep, log, mid = _sharded_run(ctx, monkeypatch, name, window, n_shards)
    dev = lsc.check_params_only(before, after, rep, lsc.case_options(name), mid=mid, log=log, bars=None, where="GPU sharded %s %s %d" % (name, window, n_shards))
    _hold("sharded %s %s %d" % (name, window, n_shards), dev)


def test_sharded_step_over_a_one_rank_communicator(ctx, monkeypatch):
    """Window 7400 over four shards: the RCCL exchange on a communicator of one rank gives the bytes of the virtual-shard run, and
    both pass the check."""
    _set_path(monkeypatch, {})
    w = lsc.sharded_window("7400")
    ctx_r = ba.Context(0)
    try:
        ctx_r.comm_init(ctx_r.comm_unique_id(), 0, 1)
        for name in ("default", "two_steps"):
            o = lsc.case_options(name)
            one = lsc.one_step_options(o) if o.max_num_iterations == 2 else None
            av, rv, lv = _sharded(ctx, w, o, 4)
            ar, rr, lr = _sharded(ctx_r, w, o, 4)
            assert lsc.same_bytes(ar, av) and [rr[k] for k in REPORT_KEYS] == [rv[k] for k in REPORT_KEYS], name
            mid = _sharded(ctx_r, w, one, 4)[0] if one else None
            assert mid is None or lsc.same_bytes(mid, _sharded(ctx, w, one, 4)[0]), name
            dev = lsc.check_params_only(w, ar, rr, o, mid=mid, log=lr, bars=None, where="GPU sharded RCCL %s" % name)
            _hold("sharded 7400 4 one-rank RCCL " + name, dev)
    finally:
        ctx_r.close()
