"""The two layouts of the Schur partial slabs against each other, bit by bit (kba_items.hpp:slab_packed_write / cam_solve).

The one-launch solve (k_solve_coop) keeps 16 x 16 tiles of an nf_pad x nf_pad matrix per slab; the lock-step launches
(KBA_NO_COOP_SOLVE=1) and the streaming solve (KBA_STREAM_MIN=1) store the slabs of fast-class windows packed: the entries the camera
solve reads, back to back, a plain slab for the pose slots only.  Same slabs, same summation chains, same additions: poses, plane
parameters, landmarks, trimmed sets and every integer and cost field of the report must be the same bytes whichever path solves a
window, alone or inside a batch.

Shapes - the smallest at which the packing can go wrong (landmarks before the selection of synth.make_window; a Schur block is 64
landmarks of one class, a plain slab two blocks, a ground-plane slab one):
  * 1, 2, 3, 4 free keyframes (6 .. 24 pose slots: the single-tile and the two-tile epilogue of the plain Schur wave);
  * no free plane slot and no ground-plane slab (with_ground_plane=False);
  * no plain slab (every landmark carries a ground-plane row);
  * one plain slab (fewer than four: an entry with a plane slot starts its sum at slab 0 and meets plain slabs that have no such
    entry), three, and five (not a multiple of four: 700 landmarks - the one shape above 400, the smallest with more than four);
  * a last Schur block of one landmark (65 plain landmarks);
  * trimming on (more than 100 landmarks) and off (the 65-landmark windows trim nothing).
"""
import numpy as np
import pytest

from limo_amd import ba, default_options, synth

pytestmark = pytest.mark.gpu

CASES = [
    dict(seed=7200, n_kf=2, n_lm=400),
    dict(seed=7201, n_kf=3, n_lm=400),
    dict(seed=7202, n_kf=4, n_lm=400),
    dict(seed=7203, n_kf=5, n_lm=400),
    dict(seed=7204, n_kf=5, n_lm=300, with_ground_plane=False),
    dict(seed=7205, n_kf=3, n_lm=300, with_ground_plane=False),
    dict(seed=7102, n_kf=4, n_lm=200, ground_frac=1.0),
    dict(seed=7100, n_kf=5, n_lm=150),
    dict(seed=7101, n_kf=5, n_lm=700),
    dict(seed=7103, n_kf=3, n_lm=65, with_ground_plane=False),
    dict(seed=7102, n_kf=3, n_lm=65),
]
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "n_depth_blocks", "n_repr_blocks",
               "n_gp_blocks", "n_trimmed_landmarks", "num_linearizations", "initial_cost", "final_cost")
_ENV = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN")


def _window(c):
    return synth.make_window(c["seed"], **{k: v for k, v in c.items() if k != "seed"})


def _plain_slabs(w):
    n_plain = int(w.n_lm - w.lm_is_ground.sum())
    return ((n_plain + 63) // 64 + 1) // 2


def _solve(ctx, windows, monkeypatch, env, path, prepare=None):
    """Results of one ba.Batch of copies of `windows`: per window (report fields, parameter bytes, trimmed set).  `path`: the launch
    path the solve has to report (limo_ctx_last_solve_info)."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b = ba.Batch(ctx, [w.copy() for w in windows])
    if prepare is not None:
        prepare(b, monkeypatch)
    b.solve(default_options())
    info = ctx.last_solve_info()
    assert info["path"] == path and info["recovered"] == 0, (env, info)
    reps = b.download()
    out = []
    for i, w in enumerate(b.windows):
        out.append((tuple(reps[i][k] for k in REPORT_KEYS), w.kf_pose.tobytes(), w.kf_plane_dir.tobytes(), w.kf_plane_dist.tobytes(), w.lm_pos.tobytes(),
                    b.trimmed(i).tobytes()))
    b.close()
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    return out


_tile = {}  # case index -> result of the one-launch solve (tile layout): computed once, shared, never changed


def _tile_result(ctx, i, monkeypatch):
    if i not in _tile:
        _tile[i] = _solve(ctx, [_window(CASES[i])], monkeypatch, {}, "COOP")[0]
    return _tile[i]


def _same(a, b, what):
    assert a[0] == b[0], (what, dict(zip(REPORT_KEYS, a[0])), dict(zip(REPORT_KEYS, b[0])))
    for name, x, y in zip(("kf_pose", "kf_plane_dir", "kf_plane_dist", "lm_pos", "trimmed"), a[1:], b[1:]):
        assert x == y, (what, name)


def test_shapes_are_what_the_cases_are_for():
    ws = [_window(c) for c in CASES]
    assert [w.n_kf - 1 for w in ws[:4]] == [1, 2, 3, 4]
    assert all(_plain_slabs(w) == 3 for w in ws[:4])
    assert ws[4].lm_is_ground.sum() == 0 and ws[6].lm_is_ground.all()
    assert _plain_slabs(ws[7]) == 1 and ws[7].lm_is_ground.sum() > 0
    assert _plain_slabs(ws[8]) == 5 and ws[8].lm_is_ground.sum() > 64  # ... and more than one ground-plane slab
    assert ws[9].n_lm == 65 and ws[9].lm_is_ground.sum() == 0           # blocks of 64 + 1 landmarks
    assert all(w.n_lm <= 400 for i, w in enumerate(ws) if i != 8)
    assert sum(w.n_lm > 100 for w in ws) >= 8 and sum(w.n_lm <= 100 for w in ws) == 2  # trimming on / off


@pytest.mark.parametrize("i", range(len(CASES)))
def test_lock_step_packed_equals_one_launch_tiles(ctx, i, monkeypatch):
    got = _solve(ctx, [_window(CASES[i])], monkeypatch, {"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}, "LOCKSTEP")[0]
    _same(_tile_result(ctx, i, monkeypatch), got, CASES[i])
    if CASES[i]["n_lm"] > 100:
        assert got[0][REPORT_KEYS.index("num_solves")] >= 2  # the trimming solves ran
    else:
        assert got[0][REPORT_KEYS.index("n_trimmed_landmarks")] == 0


def test_streaming_batch_packed_equals_one_launch_tiles(ctx, monkeypatch):
    ws = [_window(c) for c in CASES]
    got = _solve(ctx, ws, monkeypatch, {"KBA_STREAM_MIN": "1"}, "STREAMING")
    for i in range(len(CASES)):
        _same(_tile_result(ctx, i, monkeypatch), got[i], CASES[i])


@pytest.mark.parametrize("i", [3, 7])
def test_one_launch_solve_after_a_packed_solve_of_the_same_batch(ctx, i, monkeypatch):
    """The tile layout counts on the zeros of the allocation in tiles a plain group never writes; packed slabs of an earlier solve of
    the SAME batch lie across them.  Lock-step solve, reset, one-launch solve: the bits of a fresh batch's one-launch solve."""
    def prepare(b, mp):
        b.solve(default_options())  # (KBA_NO_COOP_SOLVE is set: packed)
        assert ctx.last_solve_info()["path"] == "LOCKSTEP"
        b.reset()
        mp.delenv("KBA_NO_COOP_SOLVE")
        mp.delenv("KBA_NO_WG_SOLVE")

    got = _solve(ctx, [_window(CASES[i])], monkeypatch, {"KBA_NO_COOP_SOLVE": "1", "KBA_NO_WG_SOLVE": "1"}, "COOP", prepare)[0]
    _same(_tile_result(ctx, i, monkeypatch), got, CASES[i])
