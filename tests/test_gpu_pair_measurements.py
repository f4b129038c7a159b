"""The measurements at the pair's index (kba_layout.hpp:BatchView::pair_m) on the GPU.  k_lin_lm and k_backsub (and the one-launch kernels
that run the same device functions) read a pair's u, v, d from three planes indexed like lm_slot instead of through the slot table, tell a
pair the landmark does not have by the depth plane's missing-pair value, and k_backsub's plane loads take no slot either.  A batch through
the launch sequences against each window's single cooperative launch, bit for bit, and every shape against the oracle.  Every path runs
the same lane arithmetic (the planes' scalars are loaded everywhere, none rebuilt), so the byte comparison holds the INDEXING - landmark
offsets inside a batch, Vmax above a window's views, the planes' padding - not two ways of computing a value; what is computed is held by
the oracle.  The stereo window (two views per keyframe) is not taken by the cooperative kernel: its single call is a launch sequence as
well, and only its place in the batch and the oracle's tolerance hold it.  The device-side fill of the planes (k_pair_fill) has no
download of its own; a wrong entry moves a result here and in every solve of the tier.  The shapes
(tests/pair_meas_common.py) are small windows where the indexing can go wrong: 2 / 3 / 5 keyframes, 63 / 65 / 257 / 300 landmarks, two
views per keyframe, first / last views missing, landmarks of one view, non-positive caller depths (-2, the planes' own missing-pair
value, among them), constant landmarks, a window that trims."""
import numpy as np
import pytest

import fixed_lm_common as flc
import pair_meas_common as pmc
from limo_amd import ba, default_options

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_ba.py: pose translations and final cost against the oracle
SHAPES = pmc.shapes()
NAMES = sorted(SHAPES)
PATH_SWITCHES = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_COOP_MAX_WIN", "KBA_GROUPS", "KBA_COOP_TIMEOUT_MS")
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "num_linearizations",
               "n_depth_blocks", "n_repr_blocks", "n_gp_blocks", "n_trimmed_landmarks", "initial_cost", "final_cost")


def _force(monkeypatch, path):
    """The launch path of the next solves, the way tests/test_gpu_fixed_landmarks.py forces them."""
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


def _solve_batch(ctx, windows, flag_list, o):
    b = ba.Batch(ctx, [w.copy() for w in windows], lm_fixed=flag_list)
    b.solve(o)
    reps = b.download()
    st = _state(b, reps)
    b.close()
    return st


@pytest.fixture(scope="module")
def single(ctx):
    """Every shape as its own call, through k_solve_coop where the cooperative kernel takes the window."""
    o = default_options()
    out, paths = {}, {}
    with pytest.MonkeyPatch.context() as mp:
        _force(mp, "COOP")
        for name in NAMES:
            w, flags = SHAPES[name]
            out[name] = _solve_batch(ctx, [w], None if flags is None else [flags], o)[0]
            paths[name] = ctx.last_solve_info()["path"]
    return out, paths


def test_single_calls_take_the_cooperative_kernel(single):
    _, paths = single
    for name in NAMES:
        if not name.startswith("stereo"):
            assert paths[name] == "COOP", (name, paths[name])


@pytest.mark.parametrize("path", ["STREAMING", "LOCKSTEP"])
def test_batch_through_the_launch_sequence_equals_the_single_calls(ctx, single, monkeypatch, path):
    """All shapes as one batch (landmark offsets that are no multiple of 64, Vmax = 6 for windows of 2 - 5 views): reports, parameters and
    trimmed sets of every window byte-equal to its single call."""
    want, _ = single
    o = default_options()
    _force(monkeypatch, path)
    ws, fl = [SHAPES[k][0] for k in NAMES], [SHAPES[k][1] for k in NAMES]
    got = _solve_batch(ctx, ws, fl, o)
    assert ctx.last_solve_info()["path"] == path
    for name, g in zip(NAMES, got):
        x = want[name]
        assert g[0] == x[0], (path, name, dict(zip(REPORT_KEYS, g[0])), dict(zip(REPORT_KEYS, x[0])))
        assert all(np.array_equal(p, q) for p, q in zip(g[1:], x[1:])), (path, name)
    assert want["trim_400"][0][REPORT_KEYS.index("n_trimmed_landmarks")] > 0 and all(x[0][REPORT_KEYS.index("iterations_total")] > 0 for x in want.values())


@pytest.mark.parametrize("name", NAMES)
def test_shapes_match_the_oracle(ctx, oracle, single, name):
    """tests/test_gpu_ba.py's bar (check_solve_parity): block counts, trimmed count, initial cost to 1e-9, final cost and keyframe translations to
    1e-4 - against the oracle, for windows with constant landmarks against the oracle with those blocks set constant."""
    w, flags = SHAPES[name]
    o = default_options()
    rep, kf_pose, _, _, lm_pos, trimmed = single[0][name]
    rg = dict(zip(REPORT_KEYS, rep))
    wo = w.copy()
    if flags is None:
        ro, _ = oracle.solve(wo, o)
    else:
        ro, to = flc.ref_solve(wo, flags, o)
        assert np.array_equal(np.sort(trimmed), to)
        assert np.array_equal(lm_pos[flags != 0], w.lm_pos[flags != 0])  # constant landmarks come back bit for bit
    print("%s: final cost %.9g / %.9g, iterations %d / %d, trimmed %d" % (name, rg["final_cost"], ro["final_cost"], rg["iterations_total"], ro["iterations_total"], rg["n_trimmed_landmarks"]))
    assert rg["n_depth_blocks"] == ro["n_depth_blocks"] and rg["n_gp_blocks"] == ro["n_gp_blocks"]
    assert rg["n_trimmed_landmarks"] == ro["n_trimmed_landmarks"]
    assert abs(rg["initial_cost"] - ro["initial_cost"]) <= 1e-9 * abs(ro["initial_cost"])
    assert abs(rg["final_cost"] - ro["final_cost"]) <= TOL * abs(ro["final_cost"])
    assert np.abs(kf_pose[:, 4:] - wo.kf_pose[:, 4:]).max() / max(1e-12, np.abs(wo.kf_pose[:, 4:]).max()) <= TOL
    assert np.array_equal(kf_pose[0], w.kf_pose[0])  # keyframe 0 is Pose-fixed
