"""One LM step of the windowed solve on the GPU against the dense reference of tests/lm_step_common.py, option by option.

What a step runs - k_lin_lm, the Schur waves, k_cam_assemble, k_cam_solve, k_backsub - is otherwise held to byte identity between
launch paths and to the oracle after tens of iterations, and neither sees a slightly wrong linear system.  Here a solve of ONE
iteration (two where the case is about the second step) with the iteration log on is compared with x0 (+) delta of a dense
least-squares solve and with the scalars of Ceres' table, under the bars the CPU tier sets (lm_step_common.BARS: 100 x the spread of
the emulator and the oracle; tests/test_lm_step_cpu.py):
  * twelve shapes at the default options and with jacobi_scaling = 0: the nine windows of test_gpu_schur_head.py (1 .. 4 free
    keyframes, an odd number of plain Schur blocks, a last block of one landmark, a ground-plane class of fewer than 16 landmarks,
    only / no ground-plane landmarks, a free keyframe without a view), a stereo window, one with a depth on every measurement and
    one without any depth or ground plane;
  * every solver option off its default on the four small windows (lm_step_common.OPTION_CASES), one resident batch per option set;
  * the default path of such a batch against the reference, and for four sets the lock-step and the streaming path against the
    default path: same bytes for parameters, report and log.
The GPU's own deviation per class is printed by every test (pytest -s) and recorded in profiles/lm_step_reference.md."""
import contextlib

import pytest

import lm_step_common as lsc
from limo_amd import ba

pytestmark = pytest.mark.gpu

_ENV = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_NO_SCHUR_PAIR")
PATHS = {"default": {}, "LOCKSTEP": {"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}, "STREAMING": {"KBA_STREAM_MIN": "1"}}
PATH_CASES = ("default", "min_diag_unscaled", "min_relative_decrease_10", "two_steps")  # the sets that also run the other two paths
REPORT_KEYS = lsc.REPORT_INTS + ("initial_cost", "final_cost")
CASES = lsc.all_cases()

_cache = {}  # (case name, path) -> the batch's results: computed once, shared, never changed


@contextlib.contextmanager
def _iteration_log(ctx):
    ctx.set_iteration_log(True)
    try:
        yield
    finally:
        ctx.set_iteration_log(False)


def _solve(ctx, seeds, o):
    """One resident batch of the windows of `seeds` under `o`: [(after, report, log)] and the path the solve took."""
    b = ba.Batch(ctx, [lsc.window(s) for s in seeds])
    try:
        b.solve(o)
        reps = b.download()
        out = [(b.windows[i], reps[i], b.iteration_log(i)) for i in range(len(seeds))]
        return out, ctx.last_solve_info()
    finally:
        b.close()


def _runs(ctx, monkeypatch, name, path):
    """seed -> (after, report, log, mid) of the batch of a case on a launch path (mid: the batch's result after ONE iteration where
    the case takes two)."""
    if (name, path) not in _cache:
        for k in _ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in PATHS[path].items():
            monkeypatch.setenv(k, v)
        o = lsc.case_options(name)
        seeds = [s for n, s in CASES if n == name]
        with _iteration_log(ctx):
            out, info = _solve(ctx, seeds, o)
            mids = _solve(ctx, seeds, lsc.one_step_options(o))[0] if o.max_num_iterations == 2 else [(None,)] * len(seeds)
        assert info["recovered"] == 0 and (path == "default" or info["path"] == path), (name, path, info)
        for k in _ENV:
            monkeypatch.delenv(k, raising=False)
        _cache[name, path] = {s: r + (m[0],) for s, r, m in zip(seeds, out, mids)}
    return _cache[name, path]


@pytest.mark.parametrize("name,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_step_against_the_dense_reference(ctx, monkeypatch, name, seed):
    after, rep, log, mid = _runs(ctx, monkeypatch, name, "default")[seed]
    dev = lsc.check_step(lsc.window(seed), after, rep, log, lsc.case_options(name), mid=mid, bars=None, where="GPU %s %d" % (name, seed))
    print("GPU deviation", name, seed, {c: "%.2e" % v for c, v in sorted(dev.items())})  # (printed before it is held to the bars)
    for cls, v in dev.items():
        assert v <= lsc.BARS[cls], (name, seed, cls, "%.3e > %.1e" % (v, lsc.BARS[cls]))


@pytest.mark.parametrize("path", ["LOCKSTEP", "STREAMING"])
@pytest.mark.parametrize("name", PATH_CASES)
def test_same_bytes_on_every_launch_path(ctx, monkeypatch, name, path):
    want = _runs(ctx, monkeypatch, name, "default")
    got = _runs(ctx, monkeypatch, name, path)
    assert list(got) == list(want)
    for seed in want:
        for a, b in ((want[seed][0], got[seed][0]), (want[seed][3], got[seed][3])):
            assert (a is None and b is None) or lsc.same_bytes(a, b), (name, path, seed)
        assert [got[seed][1][k] for k in REPORT_KEYS] == [want[seed][1][k] for k in REPORT_KEYS], (name, path, seed)
        assert len(got[seed][2]) == len(want[seed][2]) and got[seed][2].tobytes() == want[seed][2].tobytes(), (name, path, seed)
