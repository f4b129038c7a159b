"""A parameter sweep in lock step on the emulated backend (apps/limo_stream --sequences N --sweep FILE; the second constructor of
limo_amd/kba/lockstep_driver.hpp): every sequence drives the same world with outlier-rejection parameters of its own, and its pose
file is the single drive with those parameters as flags, BYTE FOR BYTE.  The emulated C-ABI has no batched entry point of the bundle
adjustment at all, so the pose-only and solve stages fall back to one call per job here - each with the job's OWN options, which is
what this tier pins (the batched calls with an entry of options per window: tests/test_gpu_window_options.py).  Runs on the
stand-alone build under the address and undefined-behaviour sanitizers.  In the same file: the two new symbols of the C-ABI are
exported and bound, and the ABI version has not moved."""
import os
import subprocess

import pytest

import lockstep_common as lc

SWEEP = (
    "depth_thres=0.08 reprojection_thres=3.0 outlier_quantile=0.8 shrubbery_weight=0.5",
    "depth_thres=0.4 window=4",
    "reprojection_thres=0.8 outlier_quantile=0.9",
)
FLAGS = (
    ["--depth-thres", "0.08", "--reprojection-thres", "3.0", "--outlier-quantile", "0.8", "--shrubbery-weight", "0.5"],
    ["--depth-thres", "0.4", "--window", "4"],
    ["--reprojection-thres", "0.8", "--outlier-quantile", "0.9"],
)
BASE = ["--sequences", "3", "--frames", "24", "--az", "2000", "--seed", "7"]


@pytest.fixture(scope="module")
def exe():
    return lc.build_asan()


def test_a_sweep_equals_its_single_drives_with_flags(exe, tmp_path):
    sweep = tmp_path / "sweep.txt"
    sweep.write_text("\n".join(SWEEP) + "\n")
    info, files = lc.run_lockstep(exe, BASE + ["--sweep", str(sweep)], str(tmp_path / "sweep_poses"), timeout=900)
    assert info["sequences"] == 3 and info["frames"] == 72
    for i, flags in enumerate(FLAGS):
        rows, _ = lc.single_rows(exe, 24, 7, ["--az", "2000"] + flags, tmp_path, timeout=900)  # (seed 7 for all: one world)
        assert files[i] == rows, "sequence %d" % i
    default_rows, _ = lc.single_rows(exe, 24, 7, ["--az", "2000"], tmp_path, timeout=900)
    assert len(set(files)) == 3 and default_rows not in files  # (the parameters act: three different drives, none the default one)
    # the per-sequence part echoes the parameters next to the ATE; missing keys took the command line's (default) value
    ps = info["per_sequence"]
    assert [(p["depth_thres"], p["reprojection_thres"], p["outlier_quantile"], p["shrubbery_weight"], p["window"]) for p in ps] == [
        (0.08, 3.0, 0.8, 0.5, 5), (0.4, 1.6, 0.95, 0.9, 4), (0.16, 0.8, 0.9, 0.9, 5)]
    assert all(p["seed"] == 7 and p["ate_rmse"] < 0.05 for p in ps)
    # no batched bundle-adjustment entry point on this backend: every job was a single call, none carried another window's options
    for name in ("pose_only", "solve"):
        st = info["stages"][name]
        assert st["batched_calls"] == 0 and st["per_window_calls"] == 0 and st["fallback_calls"] > 0, name


def test_command_line_values_fill_the_missing_keys(exe, tmp_path):
    sweep = tmp_path / "sweep.txt"
    sweep.write_text("depth_thres=0.4\n\nwindow=4\n")  # (an empty line is no sequence)
    info, files = lc.run_lockstep(exe, ["--sequences", "2", "--frames", "12", "--az", "2000", "--seed", "7", "--reprojection-thres", "3.0", "--sweep", str(sweep)],
                                  str(tmp_path / "fill"), timeout=900)
    assert [(p["depth_thres"], p["reprojection_thres"], p["window"]) for p in info["per_sequence"]] == [(0.4, 3.0, 5), (0.16, 3.0, 4)]
    rows, _ = lc.single_rows(exe, 12, 7, ["--az", "2000", "--reprojection-thres", "3.0", "--depth-thres", "0.4"], tmp_path, timeout=900)
    assert files[0] == rows


def test_refusals(exe, tmp_path):
    def run(args):
        return subprocess.run([exe] + args + ["--quiet", "--poses", str(tmp_path / "P")], capture_output=True, text=True, timeout=900)

    sweep = tmp_path / "bad.txt"
    sweep.write_text("depth_thres=0.1\nmax_num_iterations=50\n")
    r = run(["--sequences", "2", "--frames", "4", "--sweep", str(sweep)])
    assert r.returncode == 2 and "unknown key `max_num_iterations`" in r.stderr and "line 2" in r.stderr
    sweep.write_text("depth_thres=0.1\n")
    r = run(["--sequences", "2", "--frames", "4", "--sweep", str(sweep)])
    assert r.returncode == 2 and "1 lines for 2 sequences" in r.stderr
    sweep.write_text("depth_thres=abc\ndepth_thres=0.1\n")
    assert run(["--sequences", "2", "--frames", "4", "--sweep", str(sweep)]).returncode == 2
    assert run(["--frames", "4", "--sweep", str(sweep)]).returncode == 2  # --sweep goes with --sequences
    # a field that decides the schedule of a batched solve may not differ between the sequences
    r = run(["--sequences", "3", "--frames", "4", "--perturb-trim-rounds", "2"])
    assert r.returncode == 2 and "sequence 2" in r.stderr and "outlier_rejection_num_iterations" in r.stderr
    assert not os.path.exists(str(tmp_path / "P.0"))


def test_the_new_symbols_are_exported_and_bound():
    import ctypes as C

    from limo_amd import _ffi

    lib = _ffi.load()
    assert lib.limo_abi_version() == 6 == _ffi.ABI_VERSION
    for name in ("limo_ba_batch_solve_each", "limo_ba_adjust_pose_only_batch_each"):
        assert name in _ffi.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert lib.limo_ba_batch_solve_each.argtypes == [C.c_void_p, C.c_int32, C.POINTER(_ffi.BaOptions)]
    assert lib.limo_ba_adjust_pose_only_batch_each.argtypes == [C.c_void_p, C.c_int32, C.POINTER(_ffi.BaWindow), C.POINTER(_ffi.SpeedPrior),
                                                               C.POINTER(_ffi.BaOptions), C.POINTER(_ffi.BaReport)]
    # NULL arguments are refused without a device (nothing is dereferenced, nothing launched)
    assert lib.limo_ba_batch_solve_each(None, 1, None) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_ba_adjust_pose_only_batch_each(None, 1, None, None, None, None) == _ffi.LIMO_ERR_INVALID
