"""The lock-step drive on the emulated backend (apps/limo_stream --sequences, limo_amd/kba/lockstep_driver.hpp): the pose file of
sequence i is the pose file of the single drive with the same seed and frame count, BYTE FOR BYTE - whatever the stagger, the frame
counts and the number of host threads.  The emulated C-ABI has no batched entry point, so every stage loops over its single call
here (the counts say so); what this tier pins is the host side: the split-phase shim, the order of the stages, the per-sequence state.
The stand-alone sanitized builds run the first case as host programs of their own."""
import os
import subprocess

import pytest

import emu_ffi
import lockstep_common as lc


@pytest.fixture(scope="module")
def exe():
    return emu_ffi.build_stream_app(gpu=False)


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    return tmp_path_factory.mktemp("lockstep")


@pytest.fixture(scope="module")
def first_case(exe, shared):
    return lc.run_lockstep(exe, lc.FIRST_CASE, str(shared / "first"))


def singles(exe, shared, frames_and_seeds, extra):
    return [lc.single_rows(exe, f, s, ["--az", "2000"] + extra, shared) for f, s in frames_and_seeds]


def test_staggered_sequences_of_different_length_match_their_single_drives(exe, shared, first_case):
    info, files = first_case
    want = singles(exe, shared, [(24, 7), (20, 8), (16, 9)], [])
    assert info["sequences"] == 3 and info["ticks"] == 24 and info["frames"] == 60
    for i, (rows, _) in enumerate(want):
        assert len(files[i].splitlines()) == (24, 20, 16)[i]
        assert files[i] == rows, "sequence %d" % i
    assert len({bytes(f[:2000]) for f in files}) == 3  # (three different drives, not one three times)
    # the solve ticks of neighbouring sequences are out of phase and the sequences end on different ticks: some tick carried a push of
    # more than one sequence, and no tick had all three solve at once more often than their shortest drive allows
    assert info["stages"]["landmark_init"]["max_items"] >= 2
    assert [s["frames"] for s in info["per_sequence"]] == [24, 20, 16] and [s["first_tick"] for s in info["per_sequence"]] == [0, 1, 2]
    assert all(s["ate_rmse"] < 0.05 for s in info["per_sequence"])


def test_host_threads_do_not_change_a_byte(exe, shared, first_case):
    _, files = first_case
    for threads in (1, 3):
        info, other = lc.run_lockstep(exe, lc.FIRST_CASE + ["--host-threads", str(threads)], str(shared / ("threads%d" % threads)))
        assert info["host_threads"] == threads
        assert other == files, "--host-threads %d" % threads


def test_one_sequence_is_the_single_drive(exe, shared):
    info, files = lc.run_lockstep(exe, ["--sequences", "1", "--frames", "24", "--az", "2000", "--seed", "7"], str(shared / "one"))
    assert info["sequences"] == 1 and info["host_threads"] == 1
    assert files[0] == singles(exe, shared, [(24, 7)], [])[0][0]


@pytest.mark.parametrize("flags", [["--five-point-prior"], ["--no-depth"]], ids=["five_point_prior", "no_depth"])
def test_variants_match_their_single_drives(exe, shared, flags):
    info, files = lc.run_lockstep(exe, ["--sequences", "3", "--frames", "16", "--stagger", "1", "--az", "2000", "--seed", "7"] + flags, str(shared / ("variant" + flags[0])))
    want = singles(exe, shared, [(16, 7), (16, 8), (16, 9)], flags)
    for i, (rows, _) in enumerate(want):
        assert files[i] == rows, "sequence %d with %s" % (i, flags)
    if flags == ["--five-point-prior"]:  # the emulated backend has no device estimator: every estimate is the host's
        calls = sum(s["five_point_calls"] for s in info["per_sequence"])
        assert calls > 0 and info["five_point_host"] == calls and info["stages"]["five_point"]["items"] == info["stages"]["five_point"]["fallback_calls"] == 0
    else:
        assert info["stages"]["depth"]["items"] == info["stages"]["depth"]["fallback_calls"] == 0


def test_a_differing_rig_is_refused(exe, tmp_path):
    r = subprocess.run([exe] + lc.FIRST_CASE + ["--perturb-rig", "1", "--quiet", "--poses", str(tmp_path / "P")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2
    assert "rig of sequence 1 differs" in r.stderr
    assert not os.path.exists(str(tmp_path / "P.0"))
    # the lock-step options without --sequences, and options the lock-step drive does not have, are refused as well
    assert subprocess.run([exe, "--stagger", "1", "--frames", "3"], capture_output=True, timeout=600).returncode == 2
    assert subprocess.run([exe, "--sequences", "2", "--frames", "3", "--progress"], capture_output=True, timeout=600).returncode == 2


def test_the_counts_add_up(exe, shared, first_case):
    info, _ = first_case
    st = info["stages"]
    want = singles(exe, shared, [(24, 7), (20, 8), (16, 9)], [])
    frames = sum(int(w[1]["frames"]) for w in want)
    keyframes = sum(int(w[1]["keyframes"]) for w in want)
    solves = sum(int(w[1]["solves"]) for w in want)
    assert frames == 60 and info["frames"] == frames
    assert sum(s["keyframes"] for s in info["per_sequence"]) == keyframes and sum(s["solves"] for s in info["per_sequence"]) == solves
    # every frame's depths, every frame's pose refinement but the first of a sequence, every push, every solve and its selection went
    # through a batched call or a single-call fallback - nothing twice, nothing dropped
    assert st["depth"]["items"] + st["depth"]["fallback_calls"] == frames
    assert st["pose_only"]["items"] + st["pose_only"]["fallback_calls"] == frames - 3
    assert st["landmark_init"]["items"] == keyframes and st["landmark_init"]["fallback_calls"] == 0 and info["landmarks_initialised"] > keyframes
    assert st["solve"]["items"] + st["solve"]["fallback_calls"] == solves
    assert st["select"]["items"] + info["select_host"] == solves  # (a refused pool counts as a fallback call AND a host selection)
    # the emulated backend serves no batched entry point but limo_landmark_init (flat over landmarks by itself)
    for name in ("depth", "five_point", "pose_only", "select", "solve"):
        assert st[name]["batched_calls"] == 0 and st[name]["items"] == 0, name
    for name in lc.STAGES:
        assert st[name]["batched_calls"] <= info["ticks"] and st[name]["max_items"] <= 3, name


def test_first_case_under_address_and_undefined_sanitizers(shared, first_case):
    exe = lc.build_asan()
    _, files = lc.run_lockstep(exe, lc.FIRST_CASE, str(shared / "asan"), timeout=900)
    assert files == first_case[1]


def test_first_case_under_thread_sanitizer(shared, first_case):
    exe = lc.build_tsan()
    if exe is None:
        pytest.skip("this toolchain has no ThreadSanitizer runtime")
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    _, files = lc.run_lockstep(exe, lc.FIRST_CASE, str(shared / "tsan"), timeout=900, env=env)
    assert files == first_case[1]
