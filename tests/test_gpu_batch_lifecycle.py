"""Lifecycles of a resident batch that cross the parts of limo_ba_batch (limo_amd/csrc/limo_batch.hpp): the slot groups of the
streaming solve torn down and rebuilt between re-solves of ONE batch, and two live batches on one context whose solves, resets and
reads interleave - nothing one batch keeps (slot groups, barrier words, iteration log, kernel timers, the per-solve record) may be
shared with the other.

The windows are the benchmark windows' shape class at the smallest size that still has all of it: 5 keyframes, about 150 landmarks
with depth and ground-plane rows - two-panel plain Schur waves, three-panel and narrow ground-plane waves, the pair launch while the
batch drains."""
import pytest

from limo_amd import ba, default_options, synth

pytestmark = pytest.mark.gpu

PATH_SWITCHES = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_COOP_MAX_WIN", "KBA_GROUPS", "KBA_COOP_TIMEOUT_MS")
STREAMING = {"KBA_STREAM_MIN": "1", "KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "num_linearizations",
               "n_depth_blocks", "n_repr_blocks", "n_gp_blocks", "n_trimmed_landmarks", "initial_cost", "final_cost")


def _windows(n, seed0):
    return [synth.make_window(seed0 + i, n_kf=5, n_lm=150) for i in range(n)]


def _switches(monkeypatch, env):
    """The launch-path switches of the next solves (the library reads them per solve)."""
    for k in PATH_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _state(b):
    """Everything a caller can read back from the batch's windows, as bytes."""
    reps = b.download()
    return [(tuple(r[k] for k in REPORT_KEYS), w.kf_pose.tobytes(), w.kf_plane_dir.tobytes(), w.kf_plane_dist.tobytes(), w.lm_pos.tobytes(),
             b.trimmed(i).tobytes()) for i, (w, r) in enumerate(zip(b.windows, reps))]


def test_slot_groups_rebuilt_between_resolves(ctx, monkeypatch):
    """Six windows, streamed with 1, 3, 2 and 1 slot groups, a reset between the solves: every change of the group count tears the
    groups' streams, events and pinned words down and builds them again on the live batch.  Same bytes from all four solves."""
    o = default_options()
    b = ba.Batch(ctx, _windows(6, 300))
    states = []
    for k, groups in enumerate((1, 3, 2, 1)):
        _switches(monkeypatch, dict(STREAMING, KBA_GROUPS=str(groups)))
        if k:
            b.reset()
        b.solve(o)
        info = ctx.last_solve_info()
        assert info["path"] == "STREAMING" and info["groups"] == groups and info["recovered"] == 0, (groups, info)
        assert info["rounds"] > 0 and info["slots"] == 6, (groups, info)
        states.append(_state(b))
    b.close()
    gp = ctx.last_schur_gp_info()
    print("rounds of the last solve %d, pair launches %d, ground-plane groups narrow %d / wide %d" % (info["rounds"], info["pair_launches"], gp["narrow_groups"], gp["wide_groups"]))
    assert states[0][0][0][REPORT_KEYS.index("iterations_total")] > 0
    for groups, s in zip((3, 2, 1), states[1:]):
        assert s == states[0], "%d slot groups" % groups


def _run_a(ctx, monkeypatch, o, after_create=lambda: None, between=lambda: None, before_download=lambda: None):
    """Batch A: four windows, streamed through one slot group, reset and streamed again.  `after_create` runs behind its creation,
    `between` behind its first solve, `before_download` behind its second.  Returns (state, kernel stats, rounds of the two solves)."""
    a = ba.Batch(ctx, _windows(4, 320))
    after_create()
    rounds = []
    for k in range(2):
        _switches(monkeypatch, dict(STREAMING, KBA_GROUPS="1"))
        if k:
            a.reset()
        a.solve(o)
        info = ctx.last_solve_info()
        assert info["path"] == "STREAMING" and info["groups"] == 1, info
        rounds.append(info["rounds"])
        if not k:
            between()
    before_download()
    out = (_state(a), a.kernel_stats(), rounds)
    a.close()
    return out


def test_two_live_batches_interleaved(ctx, monkeypatch):
    """A (four windows, streaming) and B (one window, the cooperative launch) live on one context: create A, create B, solve A,
    solve B, reset A, solve A, read B's iteration log, download both.  Every result is what the same batch gives alone on a fresh
    context, and A's kernel timers count A's launches only."""
    o = default_options()
    alone = ba.Context(0)
    alone.set_iteration_log(True)
    a_ref, a_stats_ref, a_rounds_ref = _run_a(alone, monkeypatch, o)
    alone.close()
    alone = ba.Context(0)
    alone.set_iteration_log(True)
    _switches(monkeypatch, {})
    b_alone = ba.Batch(alone, _windows(1, 340))
    b_alone.solve(o)
    assert alone.last_solve_info()["path"] == "COOP"
    b_log_ref, b_ref = b_alone.iteration_log(0), _state(b_alone)
    b_alone.close()
    alone.close()
    assert len(b_log_ref) > 0

    ctx.set_iteration_log(True)
    try:
        live = {}

        def solve_b():
            _switches(monkeypatch, {})
            live["b"].solve(o)
            info = ctx.last_solve_info()
            assert info["path"] == "COOP" and info["recovered"] == 0 and info["groups"] == 0 and info["rounds"] == 0, info

        a_state, a_stats, a_rounds = _run_a(ctx, monkeypatch, o, after_create=lambda: live.update(b=ba.Batch(ctx, _windows(1, 340))), between=solve_b,
                                            before_download=lambda: live.update(log=live["b"].iteration_log(0)))
        b_log, b_state = live["log"], _state(live["b"])
        b_stats = live["b"].kernel_stats()
        live["b"].close()
    finally:
        ctx.set_iteration_log(False)
        _switches(monkeypatch, {})
    assert a_state == a_ref
    assert b_state == b_ref
    assert b_log.tobytes() == b_log_ref.tobytes()
    # one timed linearisation launch per round of a one-group streaming solve; the cooperative launch times none
    print("A: rounds %s, linearize launches %d, Schur launches %d; B: linearize launches %d" % (a_rounds, a_stats["linearize_launches"], a_stats["schur_launches"],
                                                                                            b_stats["linearize_launches"]))
    assert a_rounds == a_rounds_ref
    assert a_stats["linearize_launches"] == sum(a_rounds) == a_stats_ref["linearize_launches"]
    assert a_stats["schur_launches"] == a_stats_ref["schur_launches"] > 0
    assert b_stats["linearize_launches"] == 0 and b_stats["schur_launches"] == 0
