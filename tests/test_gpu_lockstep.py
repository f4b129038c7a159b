"""The lock-step drive on the device (apps/limo_stream --sequences on liblimo_hip.so): one batched call per stage and tick -
limo_depth_estimate_batch, limo_five_point_batch, limo_ba_adjust_pose_only_batch, limo_landmark_init over the concatenated rays,
limo_landmark_select_batch, limo_ba_batch_create / _solve / _download - and the pose file of sequence i is the pose file of the single
GPU drive with the same seed and frame count, BYTE FOR BYTE: what include/limo_hip.h promises of every batched entry point ("window /
frame / pool i gets the bytes of its single call"), held over whole drives whose sequences start, solve and end on different ticks."""
import pytest

import emu_ffi
import lockstep_common as lc

pytestmark = pytest.mark.gpu

FOUR = ["--sequences", "4", "--frames", "80", "--frames-step", "10", "--stagger", "1", "--az", "2000", "--seed", "7"]


@pytest.fixture(scope="module")
def exe():
    return emu_ffi.build_stream_app(gpu=True)


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    return tmp_path_factory.mktemp("lockstep_gpu")


@pytest.fixture(scope="module")
def four(exe, shared):
    return lc.run_lockstep(exe, FOUR, str(shared / "four"), timeout=300)


def test_four_staggered_sequences_match_four_single_drives(exe, shared, four):
    info, files = four
    print(info)
    for i in range(4):
        rows, _ = lc.single_rows(exe, 80 - 10 * i, 7 + i, ["--az", "2000"], shared, timeout=300)
        assert len(files[i].splitlines()) == 80 - 10 * i
        assert files[i] == rows, "sequence %d" % i
    st = info["stages"]
    for name in ("depth", "pose_only", "landmark_init", "solve"):  # every call of these stages was the batched one ...
        assert st[name]["fallback_calls"] == 0, name
        assert st[name]["batched_calls"] >= 1 and st[name]["max_items"] > 1, name  # ... and some call carried more than one item
    frames = 80 + 70 + 60 + 50
    assert info["frames"] == frames and st["depth"]["items"] == frames and st["pose_only"]["items"] == frames - 4
    assert st["solve"]["items"] == sum(s["solves"] for s in info["per_sequence"]) > 0
    assert st["landmark_init"]["items"] == sum(s["keyframes"] for s in info["per_sequence"])


def test_device_selection_and_device_five_point_match_their_single_drives(exe, shared):
    flags = ["--select-device", "--five-point-prior", "--five-point-device"]
    info, files = lc.run_lockstep(exe, ["--sequences", "3", "--frames", "40", "--stagger", "1", "--az", "2000", "--seed", "7"] + flags, str(shared / "device"), timeout=300)
    print(info)
    for i in range(3):
        rows, _ = lc.single_rows(exe, 40, 7 + i, ["--az", "2000"] + flags, shared, timeout=300)
        assert files[i] == rows, "sequence %d" % i
    st = info["stages"]
    solves = sum(s["solves"] for s in info["per_sequence"])
    estimates = sum(s["five_point_calls"] for s in info["per_sequence"])
    assert st["select"]["fallback_calls"] == 0 and info["select_host"] == 0 and st["select"]["items"] == solves > 0
    assert sum(s["select_device_calls"] for s in info["per_sequence"]) == solves
    assert st["five_point"]["fallback_calls"] == 0 and info["five_point_host"] == 0 and st["five_point"]["items"] == estimates > 0
    assert st["select"]["max_items"] > 1 and st["five_point"]["max_items"] > 1


def test_the_lock_step_drive_is_reproducible(exe, shared, four):
    info, files = lc.run_lockstep(exe, FOUR, str(shared / "again"), timeout=300)
    assert files == four[1]
    assert {k: v["items"] for k, v in info["stages"].items()} == {k: v["items"] for k, v in four[0]["stages"].items()}
