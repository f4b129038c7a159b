"""limo_five_point / limo_five_point_batch on the GPU (limo_amd/csrc/five_point.hip) against the host estimator
limo_amd/kba/five_point.hpp:estimateMotion (tests/cpp/five_point_ref.cpp), BIT FOR BIT: ok, inliers, in_front, samples, E, R, t and
the inlier mask.  No tolerance anywhere: the struct's bytes are compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import five_point_common as fpc
from limo_amd import _ffi, ba

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (fpc.FOCAL, fpc.CX, fpc.CY)


@pytest.fixture(scope="module")
def ctx():
    c = ba.Context(0)
    yield c
    c.close()


def _same(got, want, where):
    for k in ("ok", "inliers", "in_front", "samples"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ("E", "R", "t"):
        assert got[k].tobytes() == want[k].tobytes(), (where, k, got[k], want[k])
    assert got["raw"] == want["raw"], where


@pytest.mark.parametrize("share", [0.1, 0.5])
@pytest.mark.parametrize("n", [5, 6, 63, 64, 65, 300, 1500])
def test_single_call_equals_the_host_estimator(ctx, n, share):
    for seed in (1, 2, 3):
        a, b = fpc.make_matches(1000 * seed + n, n, share)
        want = fpc.ref_estimate(a, b, seed=seed)
        got = ctx.five_point(a, b, *K, seed=seed, with_mask=True)
        print("n %d share %.1f seed %d: ok %d samples %d inliers %d in front %d" % (n, share, seed, want["ok"], want["samples"], want["inliers"], want["in_front"]))
        _same(got, want, (n, share, seed))
        assert got["inlier"].tobytes() == want["inlier"].tobytes(), (n, share, seed)
        assert int(got["inlier"].sum()) == got["inliers"]


def test_one_sample_only(ctx):
    a, b = fpc.make_matches(11, 300, 0.3)
    want = fpc.ref_estimate(a, b, seed=4, max_samples=1)
    got = ctx.five_point(a, b, *K, seed=4, params=ctx.five_point_params(max_samples=1), with_mask=True)
    assert want["samples"] == 1
    _same(got, want, "max_samples = 1")
    assert got["inlier"].tobytes() == want["inlier"].tobytes()


def test_fewer_than_five_matches_is_ok_zero(ctx):
    a, b = fpc.make_matches(12, 4, 0.0)
    want = fpc.ref_estimate(a, b)
    got = ctx.five_point(a, b, *K, with_mask=True)  # LIMO_OK: five_point() raises otherwise
    assert not got["ok"] and got["samples"] == 0 and got["R"].tolist() == np.eye(3).tolist() and got["t"].tolist() == [0.0, 0.0, 1.0]
    _same(got, want, "n = 4")
    assert not got["inlier"].any()
    empty = ctx.five_point(np.zeros((0, 2)), np.zeros((0, 2)), *K)
    assert not empty["ok"] and empty["raw"] == got["raw"]


def test_identical_matches(ctx):
    """All matches the same: at the principal point no sample gives a model (ok = 0 after max_samples samples); elsewhere the host
    finds one that every match fits - whatever it does, the device does the same."""
    prm = ctx.five_point_params(max_samples=100)
    for pa, pb, no_model in (((fpc.CX, fpc.CY), (fpc.CX, fpc.CY), True), ((fpc.CX, fpc.CY), (fpc.CX + 5.0, fpc.CY), True), ((700.0, 200.0), (703.0, 201.0), False)):
        a, b = np.tile([pa], (40, 1)), np.tile([pb], (40, 1))
        want = fpc.ref_estimate(a, b, seed=5, max_samples=100)
        got = ctx.five_point(a, b, *K, seed=5, params=prm, with_mask=True)
        if no_model:
            assert not want["ok"] and want["samples"] == 100 and not got["inlier"].any()
        _same(got, want, ("identical matches", pa, pb))
        assert got["inlier"].tobytes() == want["inlier"].tobytes()


def test_invalid_input_is_refused(ctx):
    a, b = fpc.make_matches(13, 50, 0.1)
    lib = ctx.lib
    prm = ctx.five_point_params()
    m = _ffi.FivePointMotion()

    def call(a_, b_, n, p=prm, focal=fpc.FOCAL, out=m):
        fr = _ffi.FivePointFrame(n, None if a_ is None else a_.ctypes.data_as(_ffi.c_double_p), None if b_ is None else b_.ctypes.data_as(_ffi.c_double_p), 1)
        return lib.limo_five_point(ctx.ptr, C.byref(fr), focal, fpc.CX, fpc.CY, None if p is None else C.byref(p), None if out is None else C.byref(out), None)

    assert call(a, b, 50) == _ffi.LIMO_OK
    for bad in (np.nan, np.inf, -np.inf):
        a2 = a.copy()
        a2[17, 1] = bad
        assert call(a2, b, 50) == _ffi.LIMO_ERR_INVALID
        assert b"frame 0" in lib.limo_last_error(ctx.ptr) and b"match 17" in lib.limo_last_error(ctx.ptr)
        b2 = b.copy()
        b2[49, 0] = bad
        assert call(a, b2, 50) == _ffi.LIMO_ERR_INVALID
    assert call(a, b, -1) == _ffi.LIMO_ERR_INVALID
    assert call(None, b, 50) == _ffi.LIMO_ERR_INVALID
    assert call(a, b, 50, p=None) == _ffi.LIMO_ERR_INVALID
    assert call(a, b, 50, out=None) == _ffi.LIMO_ERR_INVALID
    assert call(a, b, 50, focal=0.0) == _ffi.LIMO_ERR_INVALID
    for field, v in (("max_samples", 0), ("max_samples", 16385), ("chunk", -1), ("probability", 0.0), ("probability", 1.5), ("probability", float("nan")),
                     ("threshold_px", 0.0), ("threshold_px", float("inf"))):
        assert call(a, b, 50, p=ctx.five_point_params(**{field: v})) == _ffi.LIMO_ERR_INVALID, (field, v)
    # a frame of a batch: the error names it
    frames = (_ffi.FivePointFrame * 3)()
    bad = a.copy()
    bad[3, 0] = np.nan
    for i, aa in enumerate((a, a, bad)):
        frames[i] = _ffi.FivePointFrame(50, aa.ctypes.data_as(_ffi.c_double_p), b.ctypes.data_as(_ffi.c_double_p), 1)
    ms = (_ffi.FivePointMotion * 3)()
    assert lib.limo_five_point_batch(ctx.ptr, 3, frames, fpc.FOCAL, fpc.CX, fpc.CY, C.byref(prm), ms) == _ffi.LIMO_ERR_INVALID
    assert b"frame 2" in lib.limo_last_error(ctx.ptr)
    assert call(a, b, 50) == _ffi.LIMO_OK  # the context is fine afterwards


@pytest.mark.parametrize("n,share", [(300, 0.1), (300, 0.5), (65, 0.5)])
def test_result_does_not_depend_on_the_chunk(ctx, n, share):
    a, b = fpc.make_matches(77 + n, n, share)
    want = fpc.ref_estimate(a, b, seed=6)
    for chunk in (0, 1, 64, 1000):
        got = ctx.five_point(a, b, *K, seed=6, params=ctx.five_point_params(chunk=chunk), with_mask=True)
        _same(got, want, (n, share, chunk))
        assert got["inlier"].tobytes() == want["inlier"].tobytes(), chunk


def test_batch_of_ragged_frames_equals_single_calls(ctx):
    prm = ctx.five_point_params(max_samples=200)
    spec = [(300, 0.1), (4, 0.0), (65, 0.5), (1500, 0.3), (5, 0.0), (64, 0.7), (40, 0.0)]  # (matches, outlier share)
    frames = []
    for i, (n, share) in enumerate(spec):
        a, b = fpc.make_matches(500 + i, n, share)
        frames.append((a, b, 20 + i))
    frames[6] = (np.tile([[fpc.CX, fpc.CY]], (40, 1)), np.tile([[fpc.CX + 5.0, fpc.CY]], (40, 1)), 26)  # no sample gives a model
    want = [fpc.ref_estimate(a, b, seed=s, max_samples=200) for a, b, s in frames]
    assert not want[1]["ok"] and want[1]["samples"] == 0  # n = 4
    assert want[0]["ok"] and want[0]["samples"] <= 16  # stops early in the first round
    assert want[5]["ok"] and want[5]["samples"] == 200  # runs to the cap
    assert not want[6]["ok"] and want[6]["samples"] == 200  # ... without a model
    assert 16 < want[3]["samples"] <= 64 < want[2]["samples"] < 200  # stop in rounds two and three .. ten of chunk = 16
    for chunk in (0, 16):  # the library's schedule (one round here), and rounds of 16 samples: frames drop out one after the other
        p = ctx.five_point_params(max_samples=200, chunk=chunk)
        got = ctx.five_point_batch(frames, *K, params=p)
        single = [ctx.five_point(a, b, *K, seed=s, params=p) for a, b, s in frames]
        for i in range(len(frames)):
            _same(got[i], want[i], ("batch", chunk, i))
            assert got[i]["raw"] == single[i]["raw"], (chunk, i)
        again = ctx.five_point_batch(frames, *K, params=p)  # pool reuse: the same blocks, the same bytes
        assert [g["raw"] for g in again] == [g["raw"] for g in got]
    assert ctx.five_point_batch([], *K, params=prm) == []


def test_drive_with_either_estimator_gives_the_same_pose_rows(tmp_path):
    import emu_ffi

    exe = emu_ffi.build_stream_app(gpu=True)
    rows, info = {}, {}
    for name, extra in (("device", ["--five-point-device"]), ("host", ["--five-point-host"]), ("default", [])):
        path = str(tmp_path / (name + ".txt"))
        r = subprocess.run([exe, "--frames", "80", "--az", "2000", "--quiet", "--five-point-prior", "--poses", path] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows[name] = open(path, "rb").read()
        info[name] = {l.split()[0]: float(l.split()[1]) for l in r.stdout.splitlines() if len(l.split()) == 2 and l.split()[0].startswith(("five_point_", "ate_"))}
        print(name, info[name])
    assert info["device"]["five_point_calls"] >= 40 and info["device"]["five_point_device_calls"] == info["device"]["five_point_calls"]
    assert info["host"]["five_point_device_calls"] == 0 and info["host"]["five_point_calls"] == info["device"]["five_point_calls"]
    assert len(rows["device"].splitlines()) == 80
    assert rows["device"] == rows["host"] == rows["default"]
    assert info["device"]["ate_rmse"] < 0.1
