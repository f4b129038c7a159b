"""The per-iteration solver log (include/limo_hip.h:limo_ba_iteration) on the GPU: off by default and without influence on any
result, the same bytes on every launch path (k_solve_coop, k_solve_wg, streaming, lock-step) and after a recovered barrier
timeout, cleared by reset, bounded by the schedule, consistent with the report, in agreement with the oracle's own table, and printed
by the shim.  The windows, the identities and the oracle comparison: tests/iteration_log_common.py (the oracle runs in a child
process that never opens the GPU)."""
import contextlib
import os
import re
import subprocess

import numpy as np
import pytest

import iteration_log_common as ilc
from limo_amd import _ffi, ba

pytestmark = pytest.mark.gpu

PATH_SWITCHES = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_COOP_MAX_WIN", "KBA_GROUPS", "KBA_COOP_TIMEOUT_MS")
LOCKSTEP = {"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}
STREAMING = {"KBA_STREAM_MIN": "1"}
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "num_linearizations",
               "n_depth_blocks", "n_repr_blocks", "n_gp_blocks", "n_trimmed_landmarks", "initial_cost", "final_cost")


@contextlib.contextmanager
def launch_env(env):
    """The launch-path switches for the solves inside (the library reads them per call); restored afterwards."""
    saved = {k: os.environ.get(k) for k in PATH_SWITCHES}
    for k in PATH_SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@contextlib.contextmanager
def iteration_log(ctx, on=True):
    ctx.set_iteration_log(on)
    try:
        yield
    finally:
        ctx.set_iteration_log(False)


def solve_single(ctx, name, o=None, lm_fixed=None):
    """The single call of a test window (limo_ba_solve / limo_ba_adjust_pose_only): (report, window, the context's log)."""
    w, prior = ilc.window(name)
    o = o or ilc.options(name)
    rep = ctx.adjust_pose_only(w, prior, o) if name == "P" else ctx.solve(w, o, lm_fixed=lm_fixed)
    return rep, w, ctx.last_iteration_log(0)


def solve_resident(ctx, names, o):
    """The same windows as a resident batch: (batch, reports, per-window state bytes, per-window logs)."""
    ws = [ilc.window(k) for k in names]
    pose = names[0] == "P"
    b = ba.Batch(ctx, [w for w, _ in ws], pose_only=pose, priors=[p for _, p in ws] if pose else None)
    b.solve(o)
    reps = b.download()
    state = [(tuple(r[k] for k in REPORT_KEYS), w.kf_pose.tobytes(), w.kf_plane_dir.tobytes(), w.kf_plane_dist.tobytes(), w.lm_pos.tobytes(),
              b.trimmed(i).tobytes()) for i, (w, r) in enumerate(zip(b.windows, reps))]
    return b, reps, state, [b.iteration_log(i) for i in range(len(names))]


@pytest.fixture(scope="module")
def device_logs(ctx):
    """name -> (report, log) of the default single call of each test window with the switch on: computed once, shared, never changed."""
    out = {}
    with launch_env({}), iteration_log(ctx):
        for name in ilc.NAMES:
            rep, _, log = solve_single(ctx, name)
            assert ctx.last_solve_info()["path"] == ("WG" if name == "P" else "COOP")
            log.setflags(write=False)
            out[name] = (rep, log)
    return out


@pytest.mark.parametrize("name", ilc.NAMES)
def test_switch_changes_no_result(ctx, name):
    o = ilc.options(name)
    with launch_env({}):
        ctx.set_iteration_log(False)
        b, _, off, logs = solve_resident(ctx, [name], o)
        assert len(logs[0]) == 0  # switch off: both readers give n == 0
        b.close()
        rep_off, w_off, log_off = solve_single(ctx, name)
        assert len(log_off) == 0
        with iteration_log(ctx):
            b, _, on, logs = solve_resident(ctx, [name], o)
            rep_on, w_on, log_on = solve_single(ctx, name)
            assert len(logs[0]) > 0 and logs[0].tobytes() == log_on.tobytes()  # the batch reader and the context reader agree
            b.close()
        assert on == off
        assert all(rep_on[k] == rep_off[k] for k in REPORT_KEYS)
        assert w_on.kf_pose.tobytes() == w_off.kf_pose.tobytes() and w_on.lm_pos.tobytes() == w_off.lm_pos.tobytes()
        # switched off again: the next call leaves nothing to read
        _, _, log_off = solve_single(ctx, name)
        assert len(log_off) == 0


def test_same_log_on_every_launch_path(ctx, device_logs):
    o = ilc.options("A")
    with iteration_log(ctx):
        for name in ("A", "B", "C"):
            want = device_logs[name][1]
            with launch_env(LOCKSTEP):
                _, _, log = solve_single(ctx, name)
                assert ctx.last_solve_info()["path"] == "LOCKSTEP"
                assert len(log) == len(want) and log.tobytes() == want.tobytes(), (name, "LOCKSTEP")
        order = ["A", "B", "C", "B", "A"]
        with launch_env(STREAMING):
            b, reps, _, logs = solve_resident(ctx, order, o)
            assert ctx.last_solve_info()["path"] == "STREAMING"
            for i, name in enumerate(order):
                want_rep, want = device_logs[name]
                assert len(logs[i]) == len(want) and logs[i].tobytes() == want.tobytes(), (name, i, "STREAMING")
                assert all(reps[i][k] == want_rep[k] for k in REPORT_KEYS), (name, i)
            b.close()
        # pose-only: k_solve_wg (the fixture), the lock-step sequence, and three windows in one k_solve_wg launch
        want = device_logs["P"][1]
        with launch_env(LOCKSTEP):
            _, _, log = solve_single(ctx, "P")
            assert ctx.last_solve_info()["path"] == "LOCKSTEP"
            assert log.tobytes() == want.tobytes()
        with launch_env({}):
            ws = [ilc.window("P") for _ in range(3)]
            ctx.adjust_pose_only_batch([w for w, _ in ws], [p for _, p in ws], ilc.options("P"))
            assert ctx.last_solve_info()["path"] == "WG"
            for i in range(3):
                assert ctx.last_iteration_log(i).tobytes() == want.tobytes(), i
            with pytest.raises(ba.LimoError):
                ctx.last_iteration_log(3)  # window out of range


def test_recovered_barrier_timeout_leaves_only_the_redone_solve(ctx, device_logs):
    rep_want, want = device_logs["C"]
    with iteration_log(ctx):
        with launch_env({"KBA_COOP_TIMEOUT_MS": "0"}):
            rep, _, log = solve_single(ctx, "C")
            info = ctx.last_solve_info()
            assert info["recovered"] == 1 and info["path"] == "LOCKSTEP", info
        assert len(log) == len(want) and log.tobytes() == want.tobytes()
        assert all(rep[k] == rep_want[k] for k in REPORT_KEYS)
        with launch_env({}):  # (the next call takes the one-launch path again: the context's strike count is back at zero)
            _, _, log = solve_single(ctx, "C")
            info = ctx.last_solve_info()
            assert info["recovered"] == 0 and info["path"] == "COOP", info
            assert log.tobytes() == want.tobytes()


def test_second_solve_and_reset(ctx, device_logs):
    o = ilc.options("B")
    names = ["B", "C"]
    with launch_env({}), iteration_log(ctx):
        b, _, _, first = solve_resident(ctx, names, o)
        for i, k in enumerate(names):
            assert first[i].tobytes() == device_logs[k][1].tobytes(), k
        b.reset()
        assert all(len(b.iteration_log(i)) == 0 for i in range(2))  # reset alone clears the log
        b.solve(o)
        assert all(b.iteration_log(i).tobytes() == first[i].tobytes() for i in range(2))
        b.solve(o)  # a second solve without reset starts from zero entries: a warm start's few iterations, solve indices from 0
        reps = b.download()
        for i in range(2):
            again = b.iteration_log(i)
            assert len(again) > 0 and again["solve"][0] == 0 and again["iteration"][0] == 0
            assert len(ilc.split_solves(again)) == reps[i]["num_solves"] - len(ilc.split_solves(first[i]))  # (the report accumulates since the reset)
        ctx.set_iteration_log(False)  # switched off, the same batch records nothing any more
        b.reset()
        b.solve(o)
        assert all(len(b.iteration_log(i)) == 0 for i in range(2))
        with pytest.raises(ba.LimoError):
            b.iteration_log(2)
        b.close()


def test_capacity_is_the_bound_of_the_schedule(ctx):
    o = ilc.options("B")
    o.max_num_iterations = 3
    with launch_env({}), iteration_log(ctx):
        rep, _, log = solve_single(ctx, "B", o)
        solves = ilc.split_solves(log)
        assert rep["termination"] == _ffi.LIMO_NO_CONVERGENCE
        assert int(solves[-1][0]["solve_kind"]) == 2 and [int(e["iteration"]) for e in solves[-1]] == [0, 1, 2, 3]
        assert len(log) <= ilc.schedule_bound(o) == 1 * (3 + 7) + 4
        ilc.check_consistency(log, rep, o, "B, 3 iterations")
        b, reps, _, logs = solve_resident(ctx, ["A", "B", "C"], o)
        assert all(0 < len(l) <= ilc.schedule_bound(o) for l in logs)
        b.close()


@pytest.mark.parametrize("name", ilc.NAMES)
def test_device_log_identities(device_logs, name):
    rep, log = device_logs[name]
    counts = ilc.check_consistency(log, rep, ilc.options(name), name)
    print(name, "entries", len(log), "rejected", counts["rejected"], "invalid", counts["invalid"])
    if name == "A":
        assert counts["rejected"] >= 1


@pytest.mark.parametrize("name", ilc.ORACLE_NAMES)
def test_device_log_agrees_with_the_oracle_table(device_logs, name):
    table, rep_o = ilc.oracle_table(name)
    rep, log = device_logs[name]
    seen = ilc.check_against_oracle(log, table, name)
    print(name, "largest relative difference to the oracle on iterations <= 3 (no bar):", {k: "%.2e" % v for k, v in seen.items()})
    assert rep["num_solves"] == rep_o["num_solves"]


def test_fixed_landmarks(ctx):
    w, _ = ilc.window("B")
    o = ilc.options("B")
    half = (np.arange(w.n_lm) < w.n_lm // 2).astype(np.uint8)
    with launch_env({}), iteration_log(ctx):
        rep, _, log = solve_single(ctx, "B", lm_fixed=half)
        assert len(log) > 0
        ilc.check_consistency(log, rep, o, "B, first half constant")  # (cost incl. the fixed cost: initial and final cost bitwise)
        free, _, _ = solve_single(ctx, "B")
        assert rep["initial_cost"] == pytest.approx(free["initial_cost"], rel=1e-12)  # (the same blocks, some of them in the fixed cost)
        w2, _ = ilc.window("B")
        w2.kf_fixation[:] = _ffi.LIMO_FIX_POSE
        rep = ctx.solve(w2, o, lm_fixed=np.ones(w2.n_lm, np.uint8))
        assert rep["iterations_total"] == 0 and rep["termination"] == _ffi.LIMO_CONVERGENCE
        assert len(ctx.last_iteration_log(0)) == 0  # nothing to optimise: the solve ends before its first iteration
        ctx.solve_sharded(ilc.window("C")[0], ilc.options("C"), 2)
        assert len(ctx.last_iteration_log(0)) == 0  # not offered on the landmark-sharded path


def test_shim_prints_the_table(tmp_path):
    import emu_ffi

    exe = emu_ffi.build_stream_app(gpu=True)
    env = dict(os.environ, LIMO_STREAM_TRACE="1")
    for k in PATH_SWITCHES:
        env.pop(k, None)
    plain, prog = str(tmp_path / "plain.txt"), str(tmp_path / "progress.txt")
    base = [exe, "--frames", "12", "--az", "2000", "--quiet"]
    r0 = subprocess.run(base + ["--poses", plain], capture_output=True, text=True, timeout=600, env=env)
    r1 = subprocess.run(base + ["--poses", prog, "--progress"], capture_output=True, text=True, timeout=600, env=env)
    assert r0.returncode == 0 and r1.returncode == 0, r1.stderr[-2000:]
    assert open(plain).read() == open(prog).read()  # the pose rows are the same bytes
    assert "solver iterations logged" not in r0.stdout and not re.search(r"^iter\s+cost", r0.stdout, flags=re.M)
    calls = {"solve": 0, "adjustPoseOnly": 0}
    for l in r1.stderr.splitlines():
        if l.startswith("trace solve "):
            calls["solve"] += 1
        elif l.startswith("trace pose-only "):
            calls["adjustPoseOnly"] += 1
    assert calls["solve"] >= 1 and calls["adjustPoseOnly"] >= 1, calls
    lines = r1.stdout.splitlines()
    captions = [(i, l) for i, l in enumerate(lines) if re.match(r"^(solve|adjustPoseOnly): \d+ solver iterations logged$", l)]
    assert {k: sum(1 for _, l in captions if l.startswith(k + ":")) for k in calls} == calls  # a caption for every call the run reports
    n_tables = 0
    for j, (i, cap) in enumerate(captions):
        end = captions[j + 1][0] if j + 1 < len(captions) else len(lines)
        n_rows = int(cap.split()[1])
        block, rows, k = lines[i + 1 : end], 0, 0
        while k < len(block) and block[k].startswith("iter "):  # one table per solve of the schedule
            assert block[k].split() == ["iter", "cost", "cost_change", "|gradient|", "|step|", "tr_ratio", "tr_radius"]
            n_tables += 1
            k += 1
            first = True
            while k < len(block) and re.match(r"^\s*\d+\s", block[k]) and len(block[k].split()) == 7:
                f = [float(x) for x in block[k].split()]  # every row parses back to seven numbers
                assert np.isfinite(f).all()
                if first:
                    assert f[0] == 0 and f[6] == 1e4, block[k]
                else:
                    assert f[0] >= 1
                first = False
                rows += 1
                k += 1
            assert not first  # no table without its iteration 0
        assert rows == n_rows, (cap, rows)
        if cap.startswith("solve:"):
            assert n_rows > 0
    assert n_tables >= calls["solve"]
