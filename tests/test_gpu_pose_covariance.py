"""Marginal pose covariance on the GPU (include/limo_hip.h, "Pose covariance"): k_cam_cov behind every launch path, held to the dense
reference and the bars of tests/pose_cov_common.py (bars from the CPU tier alone; the MI355X's own maxima are printed here and
recorded in profiles/pose_covariance.md), and the pass held to being invisible: a solve with the switch on gives the bytes of a
solve with the switch off, now and in every later solve of the batch."""
import ctypes as C

import numpy as np
import pytest

import lm_step_common as lsc
import pose_cov_common as pcc
import test_gpu_schur_head as schur_head
from limo_amd import _ffi, ba, default_options

pytestmark = pytest.mark.gpu

OK_CASES = [n for n in pcc.cases() if pcc.expected_status(n) == pcc.OK]
_ENV = schur_head._ENV
NO_ONE_LAUNCH = {"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}
REPORT_KEYS = schur_head.REPORT_KEYS


@pytest.fixture
def cov_ctx(ctx, monkeypatch):
    """The session's context with the switch on for the length of a test, and the path switches cleared."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    ctx.set_pose_covariance(True)
    yield ctx
    ctx.set_pose_covariance(False)
    ctx.set_iteration_log(False)


def _batch(ctx, windows, problem=lsc.SOLVE):
    ws = [w.copy() for w in windows]
    if problem.pose_only:
        return ba.Batch(ctx, ws, pose_only=True, priors=[problem.prior] * len(ws))
    if problem.lm_fixed is not None:
        return ba.Batch(ctx, ws, lm_fixed=[problem.lm_fixed] * len(ws))
    return ba.Batch(ctx, ws)


def _snapshot(b, reps):
    """Everything a solve leaves behind that the pass must not touch, per window."""
    out = []
    for i, w in enumerate(b.windows):
        out.append((tuple(reps[i][k] for k in REPORT_KEYS), w.kf_pose.tobytes(), w.kf_plane_dir.tobytes(), w.kf_plane_dist.tobytes(), w.lm_pos.tobytes(),
                    b.trimmed(i).tobytes(), b.iteration_log(i).tobytes()))
    return out


def _solve_case(ctx, name, env=None, monkeypatch=None, path=None):
    """One window of a case as a batch of its own: (final window, matrix, status, trimmed)."""
    w0, o, problem = pcc.case(name)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    b = _batch(ctx, [w0], problem)
    b.solve(o)
    if path is not None:
        info = ctx.last_solve_info()
        assert info["path"] == path and info["recovered"] == 0, (name, env, info)
    b.download()
    cov, status = b.pose_covariance(0)
    out = (b.windows[0], cov, status, b.trimmed(0))
    b.close()
    for k in (env or {}):
        monkeypatch.delenv(k, raising=False)
    return out


_worst = {}


@pytest.mark.parametrize("name", OK_CASES)
def test_gpu_against_the_dense_reference(cov_ctx, name):
    final, cov, status, trimmed = _solve_case(cov_ctx, name)
    ref = pcc.reference(name, final, trimmed)
    dev = pcc.check_ok(cov, status, ref, bars=None, where=name)
    for cls, v in dev.items():
        if v > _worst.get(cls, (0.0, ""))[0]:
            _worst[cls] = (v, name)
    print(name, "block %.3e full %.3e" % (dev["block"], dev["full"]), " largest so far:", _worst)
    pcc.check_ok(cov, status, ref, where=name)


def test_rank_deficient_and_no_free_pose(cov_ctx):
    final, cov, status, _ = _solve_case(cov_ctx, "shape_%d" % pcc.RANK_DEFICIENT_SEED)
    assert status == pcc.RANK_DEFICIENT and np.isnan(cov).all()
    final, cov, status, _ = _solve_case(cov_ctx, "fixed_" + pcc.NOTHING_VARIABLE)
    assert status == pcc.NO_FREE_POSE and cov.shape == (6 * final.n_kf, 6 * final.n_kf) and not cov.any()


def test_solve_each_holds_every_window_to_its_own_options(cov_ctx):
    names = ["each_%d" % s for s in pcc.EACH_SEEDS]
    opts = [pcc.case(n)[1] for n in names]
    assert opts[0].depth_thres != opts[1].depth_thres and opts[0].reprojection_thres != opts[1].reprojection_thres
    b = _batch(cov_ctx, [pcc.case(n)[0] for n in names])
    b.solve(opts)
    b.download()
    for i, n in enumerate(names):
        cov, status = b.pose_covariance(i)
        dev = pcc.check_ok(cov, status, pcc.reference(n, b.windows[i], b.trimmed(i)), where=n)
        print(n, dev)
        # ... and not to the other window's: its reference is far away
        other = pcc.Reference(pcc.case(n)[0], b.windows[i], opts[1 - i])
        assert min(pcc.deviation(cov, other.cov, other.free).values()) > 100 * max(pcc.BARS.values()), n
    b.close()


# ------------------------------------------------------------------------------------------------ one set of bytes on every path
def test_same_bytes_on_every_launch_path_regular_window(cov_ctx, monkeypatch):
    name = "shape_7102"
    coop = _solve_case(cov_ctx, name, {}, monkeypatch, "COOP")
    lock = _solve_case(cov_ctx, name, NO_ONE_LAUNCH, monkeypatch, "LOCKSTEP")
    stream = _solve_case(cov_ctx, name, schur_head.STREAMING, monkeypatch, "STREAMING")
    assert coop[2] == lock[2] == stream[2] == pcc.OK
    assert coop[1].tobytes() == lock[1].tobytes() == stream[1].tobytes()


@pytest.mark.parametrize("name", ("pose_71", "fixed_e_all"))
def test_same_bytes_after_the_workgroup_solve(cov_ctx, monkeypatch, name):
    wg = _solve_case(cov_ctx, name, {}, monkeypatch, "WG")
    lock = _solve_case(cov_ctx, name, NO_ONE_LAUNCH, monkeypatch, "LOCKSTEP")
    assert wg[2] == lock[2] == pcc.OK and wg[1].tobytes() == lock[1].tobytes()


def test_alone_and_inside_a_batch(cov_ctx, monkeypatch):
    o = default_options()
    ws = [schur_head._window(c) for c in schur_head.CASES]
    b = _batch(cov_ctx, ws)
    b.solve(o)
    assert cov_ctx.last_solve_info()["path"] == "COOP"
    inside = [b.pose_covariance(i) for i in range(len(ws))]
    b.close()
    for k, v in schur_head.STREAMING.items():
        monkeypatch.setenv(k, v)
    b = _batch(cov_ctx, ws)
    b.solve(o)
    assert cov_ctx.last_solve_info()["path"] == "STREAMING"
    streamed = [b.pose_covariance(i) for i in range(len(ws))]
    b.close()
    for k in schur_head.STREAMING:
        monkeypatch.delenv(k)
    for i, w in enumerate(ws):
        one = _batch(cov_ctx, [w])
        one.solve(o)
        cov, status = one.pose_covariance(0)
        one.close()
        want = pcc.RANK_DEFICIENT if schur_head.CASES[i]["seed"] == pcc.RANK_DEFICIENT_SEED else pcc.OK
        assert status == inside[i][1] == streamed[i][1] == want, (i, status, inside[i][1], streamed[i][1])
        assert cov.tobytes() == inside[i][0].tobytes() == streamed[i][0].tobytes(), i
        if want == pcc.OK:
            assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes() and (np.diag(cov)[6:] > 0).all(), i


# ------------------------------------------------------------------------------------------------ the pass is invisible
@pytest.mark.parametrize("env,path", [({}, "COOP"), (NO_ONE_LAUNCH, "LOCKSTEP"), (schur_head.STREAMING, "STREAMING")])
def test_switch_on_and_off_same_solve_now_and_later(ctx, monkeypatch, env, path):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o = default_options()
    ws = [lsc.window(7300), lsc.window(7102), lsc.window(7306)]  # (fast-class windows: the default path is the cooperative launch)
    ctx.set_iteration_log(True)
    try:
        runs = {}
        for on in (False, True):
            ctx.set_pose_covariance(on)
            b = _batch(ctx, ws)
            seq = []
            b.solve(o)  # cold
            assert ctx.last_solve_info()["path"] == path
            seq.append(_snapshot(b, b.download()))
            stats = b.kernel_stats()
            status = [b.pose_covariance(i)[1] for i in range(len(ws))]
            b.solve(o)  # warm re-solve from the result
            seq.append(_snapshot(b, b.download()))
            b.reset()
            b.solve(o)  # from the reset image
            seq.append(_snapshot(b, b.download()))
            b.close()
            runs[on] = (seq, (stats["linearize_launches"], stats["schur_launches"]), status)
        assert runs[False][2] == [pcc.NOT_COMPUTED] * 3
        assert runs[True][2] == [pcc.OK, pcc.OK, pcc.RANK_DEFICIENT]
        assert runs[True][1] == runs[False][1], "the pass is not the solve's: no timed launch counted"
        for k, what in enumerate(("cold", "warm", "after reset")):
            assert runs[True][0][k] == runs[False][0][k], (path, what)
        assert runs[False][0][0][0][5] != b"" and len(runs[False][0][0][0][6]) > 0  # (the first window trims and logs: the comparison is not vacuous)
        # switched on, then off again: the next solve of the same batch reports NOT_COMPUTED
        ctx.set_pose_covariance(True)
        b = _batch(ctx, ws[:1])
        b.solve(o)
        assert b.pose_covariance(0)[1] == pcc.OK
        ctx.set_pose_covariance(False)
        b.solve(o)
        assert b.pose_covariance(0) == (None, pcc.NOT_COMPUTED)
        b.close()
    finally:
        ctx.set_pose_covariance(False)
        ctx.set_iteration_log(False)


def test_calls_that_own_their_batch(cov_ctx):
    name = "shape_7102"
    w0, o, _ = pcc.case(name)
    w = w0.copy()
    cov_ctx.solve(w, o)
    cov, status = cov_ctx.last_pose_covariance(0)
    ref = _solve_case(cov_ctx, name)
    assert status == pcc.OK and cov.tobytes() == ref[1].tobytes()
    # pose-only, single and batched with per-window priors
    wp, op, problem = pcc.case("pose_71")
    single = wp.copy()
    cov_ctx.adjust_pose_only(single, problem.prior, op)
    c1, s1 = cov_ctx.last_pose_covariance(0)
    ws = [wp.copy(), pcc.case("pose_71_none")[0], pcc.case("pose_71_small")[0]]
    cov_ctx.adjust_pose_only_batch(ws, [problem.prior, None, pcc.case("pose_71_small")[2].prior], op)
    got = [cov_ctx.last_pose_covariance(i) for i in range(3)]
    assert s1 == pcc.OK and [g[1] for g in got] == [pcc.OK] * 3
    assert got[0][0].tobytes() == c1.tobytes() == _solve_case(cov_ctx, "pose_71")[1].tobytes()
    for i, n in enumerate(("pose_71", "pose_71_none", "pose_71_small")):
        pcc.check_ok(got[i][0], got[i][1], pcc.reference(n, ws[i], ()), where=n)
    # the sharded solve offers none
    cov_ctx.solve_sharded(w0.copy(), o, 2)
    assert cov_ctx.last_pose_covariance(0) == (None, pcc.NOT_COMPUTED)
    # switch off: nothing held
    cov_ctx.set_pose_covariance(False)
    cov_ctx.solve(w0.copy(), o)
    assert cov_ctx.last_pose_covariance(0) == (None, pcc.NOT_COMPUTED)


def test_reader_arguments(cov_ctx):
    w0, o, _ = pcc.case("shape_7103")
    b = _batch(cov_ctx, [w0])
    b.solve(o)
    st = C.c_int32(-1)
    small = np.zeros(4)
    lib = cov_ctx.lib
    assert lib.limo_ba_batch_pose_covariance(b.ptr, 0, small.size, small.ctypes.data_as(_ffi.c_double_p), C.byref(st)) != 0  # too little room
    assert lib.limo_ba_batch_pose_covariance(b.ptr, 1, 0, None, C.byref(st)) != 0  # window out of range
    assert lib.limo_ba_batch_pose_covariance(b.ptr, 0, 0, None, None) != 0  # no status
    assert lib.limo_ba_batch_pose_covariance(b.ptr, 0, 0, None, C.byref(st)) == 0 and st.value == pcc.OK  # the status alone
    assert not small.any()
    b.close()
