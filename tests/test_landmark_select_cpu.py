"""The device landmark selection in the CPU tier: limo_amd/csrc/landmark_select_core.hpp - the statement the lanes of
landmark_select.hip run - serially on the host against the host classes (LandmarkSelector with cheirality + voxel + add-depth as
StreamDriver wires them), byte for byte (tests/cpp/test_landmark_select_core.cpp, a stand-alone program, also built under
-fsanitize=address,undefined); the checker library on the voxel scenario of tests/cpp/test_kba_shim.cpp; the header's symbols; the
refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import landmark_select_common as lsc
from limo_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("limo_select_default_params", "limo_landmark_select", "limo_landmark_select_batch")


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_gives_the_host_classes_bytes(which):
    plain, san = lsc.build_unit()
    r = subprocess.run([plain if which == "plain" else san], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-3000:]
    # the program checks these itself; stated here for the reader of a log: every kind of byte occurred
    m = re.search(r"(\d+) pools; checker's bytes: none (\d+) near (\d+) middle (\d+) far (\d+) must-have only (\d+) near\+must (\d+) middle\+must (\d+) far\+must (\d+) rejected (\d+)",
                  r.stdout)
    assert m and int(m.group(1)) >= 500 and all(int(g) >= 1 for g in m.groups())


def test_checker_reproduces_the_voxel_scenario_of_the_shim_test():
    """tests/cpp/test_kba_shim.cpp:test_landmark_selector_voxel (the reference's gtest LandmarkSelector.voxel): 7 landmarks, two
    near-duplicates share the voxel of their neighbour, one is 100 m off the path - 5 of 7 are selected.  The voxel scheme alone, as there."""
    lms = np.array([[0.5, 3.0, 5.5], [0.0, 100.0, 30.0], [1.0, -5.0, 4.0], [2.0, 1.0, 1.5], [-2.0, -1.0, 10.0], [-1.95, -0.99, 10.1], [0.5, 3.01, 5.52]])
    # getPoses(0, ..): translate() / rotate(angle, Z) on keyframe <- origin transforms
    T = [np.eye(4)]
    for trans, ang in (((-1.5, 0.0, -2.0), -0.05), ((-2.0, 0.0, 0.0), -0.05), ((-1.5, -0.1, 0.0), 0.0), ((-2.9, 0.0, 0.0), 0.0)):
        step = np.eye(4)
        step[:3, 3] = trans
        rot = np.eye(4)
        rot[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
        T.append(T[-1] @ step @ rot)
    kf_pose = np.zeros((5, 7))
    for k, t in enumerate(T):
        a = np.arctan2(t[1, 0], t[0, 0])
        kf_pose[k] = [np.cos(a / 2), 0, 0, np.sin(a / 2), *t[:3, 3]]
    obs = []
    for k, t in enumerate(T):
        for i, p in enumerate(lms):
            q = t[:3, :3] @ p + t[:3, 3]
            obs.append((k, i, 0, 600 * q[0] / q[2] + 300, 600 * q[1] / q[2] + 200, q[2]))
    o = np.array(obs)
    pool = {"kf_pose": kf_pose, "kf_stamp": np.arange(5), "cam": [[600, 300, 200, 1, 0, 0, 0, 0, 0, 0]], "lm_id": np.arange(7), "lm_pos": lms,
            "lm_has_depth": np.zeros(7), "lm_is_ground": np.zeros(7), "obs_kf": o[:, 0], "obs_lm": o[:, 1], "obs_cam": o[:, 2], "obs_u": o[:, 3], "obs_v": o[:, 4],
            "obs_d": o[:, 5]}
    p = lsc.params(voxel_size_xyz=(1.0, 1.0, 0.5), roi_far=30.0, roi_middle=10.0, max_near=50, max_middle=50, max_far=50)
    out = lsc.ref_select(pool, p, no_cheirality=True)
    print(out)
    assert int((out & 7 != 0).sum()) == 5
    assert out[1] == 3  # the one 100 m off lies outside the far pipe: the far field
    assert out[5] == 0 and out[6] == 0  # the near-duplicates lose their voxels to landmarks 4 and 0


def test_header_symbols_are_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "limo_hip.h")).read()
    lib = C.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, src), name
        assert name in _ffi.ABI_SYMBOLS, name
        getattr(lib, name)
    for name in ("limo_select_add", "limo_select_params", "limo_select_pool"):
        assert re.search(r"typedef struct %s \{" % name, src), name
    assert C.sizeof(_ffi.SelectAdd) == 16 and C.sizeof(_ffi.SelectParams) == 72 and C.sizeof(_ffi.SelectPool) == 16 + 8 * 13
    assert re.search(r"#define LIMO_ABI_VERSION 6\b", src)  # additive symbols: the version stays
    assert (_ffi.SELECT_HAS_DEPTH, _ffi.SELECT_IS_GROUND, _ffi.SELECT_KEY_MEASURED_DEPTH, _ffi.SELECT_KEY_RANGE) == (0, 1, 0, 1)


def test_default_params_are_the_nodes_and_a_null_context_is_refused():
    lib = _ffi.load()
    p = _ffi.SelectParams()
    lib.limo_select_default_params(C.byref(p))
    q = lsc.params()
    assert bytes(p) == bytes(q)
    assert list(p.voxel_size_xyz) == [0.5, 0.5, 0.3] and (p.roi_far, p.roi_middle, p.max_near, p.max_middle, p.max_far, p.n_add, p.sort_capacity) == (40.0, 15.0, 200, 200, 100, 0, 0)
    w, keep = _ffi.select_pool(lsc.make_pool(1, 10, 3))
    out = np.zeros(10, np.uint8)
    # device work needs a context; nothing is read through the other pointers before that is known
    assert lib.limo_landmark_select(None, C.byref(w), C.byref(p), out.ctypes.data_as(_ffi.c_uint8_p)) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_landmark_select(None, None, None, None) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_landmark_select_batch(None, 1, C.byref(w), C.byref(p), None) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_select_set_timing(None, 1) == _ffi.LIMO_ERR_INVALID


def test_checker_repeats_itself_and_the_generator_is_seeded():
    a, b = lsc.make_pool(5, 300, 3, 2), lsc.make_pool(5, 300, 3, 2)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    p = lsc.params(add=lsc.ADD, max_near=10, max_middle=25, max_far=15)
    r0, r1 = lsc.ref_select(a, p), lsc.ref_select(lsc.shuffled(b, 3), p)
    assert r0.tobytes() == r1.tobytes() and (r0 & 7 != 0).sum() > 40
