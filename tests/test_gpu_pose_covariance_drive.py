"""Marginal pose covariance through the per-frame pipeline on the device (apps/limo_stream --covariance on liblimo_hip.so): the shim's
setPoseCovariance / lastPoseCovariance behind StreamParams::pose_covariance, the Sequence's per-frame 6 x 6 of adjustPoseOnly, and the
lock-step driver's hand-over from the batched pose-only call.  The drive's pose rows must not know about the switch, every refined
frame has 36 finite numbers with status OK, and a sequence of a lock-step drive writes the bytes of its single drive."""
import os
import subprocess

import numpy as np
import pytest

import emu_ffi
import lockstep_common as lc
import pose_cov_common as pcc

pytestmark = pytest.mark.gpu

FRAMES = 40


@pytest.fixture(scope="module")
def exe():
    return emu_ffi.build_stream_app(gpu=True)


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    return tmp_path_factory.mktemp("pose_cov_drive")


_single = {}


def single_drive(exe, shared, seed):
    """(pose rows, covariance file) of the single drive with --covariance; run once per seed."""
    if seed not in _single:
        poses, cov = str(shared / ("cov_poses_%d.txt" % seed)), str(shared / ("cov_%d.txt" % seed))
        env = dict(os.environ, LIMO_STREAM_TRACE="1")  # one line per adjustPoseOnly on stderr, with the landmarks it was refined against
        r = subprocess.run([exe, "--frames", str(FRAMES), "--seed", str(seed), "--az", "2000", "--quiet", "--poses", poses, "--covariance", cov], capture_output=True,
                           text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        selected = [int(l.split(" selected ")[1].split()[0]) for l in r.stderr.splitlines() if l.startswith("trace pose-only ")]
        _single[seed] = (open(poses, "rb").read(), open(cov, "rb").read(), selected)
    return _single[seed]


def rows_of(cov_bytes):
    rows = [l.split() for l in cov_bytes.decode().splitlines()]
    assert all(len(r) == 37 for r in rows)
    return np.array([[float(x) for x in r[:36]] for r in rows]).reshape(-1, 6, 6), np.array([int(r[36]) for r in rows])


def test_single_drive_with_and_without_covariance(exe, shared):
    plain, _ = lc.single_rows(exe, FRAMES, 7, ["--az", "2000"], shared, timeout=300)
    poses, cov, selected = single_drive(exe, shared, 7)
    assert poses == plain  # the pose rows do not know about the switch
    mats, status = rows_of(cov)
    assert len(status) == FRAMES == len(plain.splitlines())
    assert status[0] == pcc.NOT_COMPUTED and not mats[0].any()  # the first frame is the origin: no adjustPoseOnly
    # every later frame runs adjustPoseOnly against the landmarks of the last selection.  Before the first solve() that selection is
    # empty: nothing constrains the pose and the honest answer is RANK_DEFICIENT; from then on the frame is refined
    assert len(selected) == FRAMES - 1
    refined = np.array([False] + [n > 0 for n in selected])
    assert refined.sum() >= FRAMES - 8, selected
    assert (status[refined] == pcc.OK).all() and (status[1:][~refined[1:]] == pcc.RANK_DEFICIENT).all(), (status, selected)
    assert np.isfinite(mats[refined]).all() and np.isnan(mats[1:][~refined[1:]]).all()
    for m in mats[refined]:
        assert (m == m.T).all() and (np.diag(m) > 0).all() and np.linalg.eigvalsh(m).min() > 0


def test_lock_step_drive_writes_the_single_drives_covariances(exe, shared):
    base = str(shared / "lockstep_poses")
    cov = str(shared / "lockstep_cov")
    info, files = lc.run_lockstep(exe, ["--sequences", "3", "--frames", str(FRAMES), "--stagger", "1", "--az", "2000", "--seed", "7", "--covariance", cov], base, timeout=300)
    st = info["stages"]["pose_only"]
    assert st["fallback_calls"] == 0 and st["max_items"] > 1  # the covariances came from the batched call
    for i in range(3):
        poses, want, _ = single_drive(exe, shared, 7 + i)
        assert files[i] == poses, "sequence %d" % i
        assert open("%s.%d" % (cov, i), "rb").read() == want, "sequence %d" % i
