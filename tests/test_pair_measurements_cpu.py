"""The measurements at the pair's index (kba_layout.hpp:BatchView::pair_m), CPU tier: what the packer writes next to lm_slot, for every
(view, landmark) of a packed batch, and that the emulated pipeline - which now reads them instead of the slot table - still computes the
bits it computed before (tests/golden/pair_measurements_emu.json)."""
import json
import os

import numpy as np
import pytest

import fixed_lm_common as flc
import pair_meas_common as pmc
from limo_amd import default_options, synth

SHAPES = pmc.shapes()


def _check_planes(t):
    """Every entry of the planes - the padding behind the last landmark and the views a window does not have included."""
    slot, pu, pv, pd = t["lm_slot"], t["pair_u"], t["pair_v"], t["pair_d"]
    assert slot.shape == pu.shape == pv.shape == pd.shape == (max(1, t["Vmax"]), t["SL"])
    miss = slot < 0
    assert np.array_equal(pu[miss], np.zeros(miss.sum(), np.float32)) and np.array_equal(pv[miss], np.zeros(miss.sum(), np.float32))
    assert not np.signbit(pu[miss]).any() and not np.signbit(pv[miss]).any()
    assert np.array_equal(pd[miss], np.full(miss.sum(), pmc.MISSING))
    s = slot[~miss]
    assert s.min() >= 0 and s.max() < t["TO"] and np.unique(s).size == s.size == t["TO"]  # every observation is some pair's, once
    assert pu[~miss].tobytes() == t["obs_u"][s].tobytes() and pv[~miss].tobytes() == t["obs_v"][s].tobytes()
    od = t["obs_d"][s]
    want = np.where(od > 0, od, pmc.NO_DEPTH).astype(np.float32)
    assert pd[~miss].tobytes() == want.tobytes()
    # no existing pair can hold the missing-pair value, and the kernels' two tests tell the three cases apart
    assert not (pd[~miss] == pmc.MISSING).any() and ((pd[~miss] > 0) == (od > 0)).all()
    # the pairs of a window lie in its own rows and columns
    for lm0, n_lm, n_view, _ in t["win"]:
        assert (slot[n_view:, lm0:lm0 + n_lm] < 0).all()
    return int((~miss).sum())


def test_every_pair_of_a_batch_holds_its_observation():
    o = default_options()
    names = sorted(SHAPES)
    ws, fl = [SHAPES[k][0] for k in names], [SHAPES[k][1] for k in names]
    t = pmc.pair_planes(ws, fl, o)
    assert t["Vmax"] == 6 and t["SL"] % 64 == 0 and t["SL"] >= t["TL"] == sum(w.n_lm for w in ws)  # (the stereo window: 3 keyframes x 2 cameras)
    assert _check_planes(t) == sum(w.n_obs for w in ws)
    # some landmark lacks its window's first view, some its last, some have one view only: the shapes are what they claim to be
    for name in ("views_257", "views_65", "const_views_65"):
        lm0, n_lm, n_view, _ = t["win"][names.index(name)]
        have = t["lm_slot"][:n_view, lm0:lm0 + n_lm] >= 0
        assert (~have[0] & have[1:].any(axis=0)).any() and (~have[n_view - 1] & have[:n_view - 1].any(axis=0)).any() and (have.sum(axis=0) == 1).any()
    # ... one window at a time, and as a batch of adjustPoseOnly problems (the same planes: state 2 landmarks read them too)
    for k in names:
        assert _check_planes(pmc.pair_planes([SHAPES[k][0]], [SHAPES[k][1]], o)) == SHAPES[k][0].n_obs
    pw = [synth.make_pose_only_case(71 + i)[0] for i in range(3)]
    assert _check_planes(pmc.pair_planes(pw, None, o, pose_only=True)) == sum(w.n_obs for w in pw)


def test_non_positive_and_nan_depths_are_pairs_without_depth():
    """Caller depths of 0, -0, -1, -2, a negative fraction, -inf and NaN: the pair exists and has no depth (kPairNoDepth) - never
    kPairMissing; obs_d keeps the caller's bits."""
    o = default_options()
    w = pmc.exact(41, 65, n_kf=3)
    vals = np.array([0.0, -0.0, -1.0, -2.0, -0.5, -np.inf, np.nan], np.float32)
    idx = np.flatnonzero(~(w.obs_d > 0))
    assert idx.size >= 2 * vals.size and (w.obs_d > 0).any()
    w.obs_d[idx] = vals[np.arange(idx.size) % vals.size]
    t = pmc.pair_planes([w], None, o)
    _check_planes(t)
    s = t["lm_slot"][t["lm_slot"] >= 0]
    pd = t["pair_d"][t["lm_slot"] >= 0]
    od = t["obs_d"][s]
    assert sorted(od.tobytes()[i:i + 4] for i in range(0, 4 * od.size, 4)) == sorted(w.obs_d.tobytes()[i:i + 4] for i in range(0, 4 * w.n_obs, 4))
    for v in vals:
        sel = np.isnan(od) if np.isnan(v) else (od == v) & (np.signbit(od) == np.signbit(v))
        assert sel.any() and (pd[sel] == pmc.NO_DEPTH).all(), v
    assert (pd[od > 0] == od[od > 0]).all()


def _golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_measurements_emu.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("n_slots", [0, 4])
def test_emulator_still_computes_the_committed_bits(n_slots):
    """Windows packed without any change of inputs solve to the bits the emulator gave before the planes existed (the golden file was
    written by the parent commit's emulator: tests/golden/make_pair_measurements_golden.py --rev) - through the lock-step and the
    streaming schedule."""
    gold = _golden()
    got = pmc.solve_all(default_options(), n_slots)
    assert sorted(got) == sorted(gold) == sorted(SHAPES)
    for name in sorted(gold):
        assert got[name] == gold[name], (name, pmc.first_difference(got[name], gold[name]))
    assert gold["trim_400"]["n_trimmed_landmarks"] > 0 and gold["kf2_63"]["n_trimmed_landmarks"] == 0  # one shape trims, one cannot
    assert all(gold[k]["iterations_total"] > 0 for k in gold)


def test_a_batch_gives_every_window_the_bits_of_its_own_solve():
    """All shapes as ONE batch (other windows' pairs in the planes' other columns, landmark offsets that are no multiple of 64)."""
    gold = _golden()
    o = default_options()
    names = sorted(SHAPES)
    ws, fl = [SHAPES[k][0].copy() for k in names], [SHAPES[k][1] for k in names]
    reps, trimmed = flc.emu_solve_batch(ws, fl, o, 0)
    for k, w, r, tr in zip(names, ws, reps, trimmed):
        got = pmc.record(w, r, tr)
        assert got == gold[k], (k, pmc.first_difference(got, gold[k]))
