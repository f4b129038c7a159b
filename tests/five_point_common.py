"""Test infrastructure of the five-point motion prior (include/limo_hip.h:limo_five_point), shared by the CPU tier
(tests/test_five_point_core_cpu.py), the GPU tier (tests/test_gpu_five_point.py) and scripts/bench_five_point.py: the stand-alone
test of limo_amd/csrc/five_point_core.hpp (tests/cpp/test_five_point_core.cpp, plain and under the sanitizers), the checker library
(tests/cpp/five_point_ref.cpp: the host estimator limo_amd/kba/five_point.hpp behind a C entry point) and the synthetic matches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from limo_amd import _ffi  # noqa: E402

_BUILD = os.path.join(_HERE, "cpp", "_build")
_CSRC = os.path.join(_ROOT, "limo_amd", "csrc")
_KBA = os.path.join(_ROOT, "limo_amd", "kba")
REF_LIB = os.path.join(_BUILD, "libfive_point_ref.so")
UNIT = os.path.join(_BUILD, "test_five_point_core")
UNIT_SAN = os.path.join(_BUILD, "test_five_point_core_san")
FOCAL, CX, CY = 718.856, 607.1928, 185.2157  # KITTI 00
_ref = None


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _headers():
    return [os.path.join(_CSRC, f) for f in ("five_point_core.hpp", "kba_math.hpp")] + [os.path.join(_KBA, f) for f in ("five_point.hpp", "definitions.hpp")] + \
        [os.path.join(_ROOT, "include", "limo_hip.h")]


def build_unit():
    """tests/cpp/test_five_point_core.cpp, plain and under -fsanitize=address,undefined (a stand-alone host program)."""
    os.makedirs(_BUILD, exist_ok=True)
    src = os.path.join(_HERE, "cpp", "test_five_point_core.cpp")
    if _stale(UNIT, [src] + _headers()):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-o", UNIT, src])
    if _stale(UNIT_SAN, [src] + _headers()):
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                               "-ffp-contract=off", "-std=c++17", "-o", UNIT_SAN, src])
    return UNIT, UNIT_SAN


def build():
    os.makedirs(_BUILD, exist_ok=True)
    src = os.path.join(_HERE, "cpp", "five_point_ref.cpp")
    if _stale(REF_LIB, [src] + _headers()):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-o", REF_LIB, src])
    build_unit()


def ref_lib():
    global _ref
    if _ref is None:
        build()
        _ref = C.CDLL(REF_LIB)
        _ref.five_point_ref_estimate.argtypes = [C.c_int32, _ffi.c_double_p, _ffi.c_double_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                                 C.c_uint64, C.c_int32, C.POINTER(_ffi.FivePointMotion), _ffi.c_uint8_p]
    return _ref


def ref_estimate(pts_a, pts_b, seed=1, probability=0.999, threshold_px=2.0, max_samples=1000, focal=FOCAL, cx=CX, cy=CY):
    """The host estimator on the matches: the Motion as a dict, with "raw" (the struct's bytes) and "inlier" (the mask)."""
    a = np.ascontiguousarray(pts_a, np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(pts_b, np.float64).reshape(-1, 2)
    m = _ffi.FivePointMotion()
    mask = np.zeros(max(1, len(a)), np.uint8)
    rc = ref_lib().five_point_ref_estimate(len(a), a.ctypes.data_as(_ffi.c_double_p), b.ctypes.data_as(_ffi.c_double_p), focal, cx, cy, probability,
                                           threshold_px, int(seed), int(max_samples), C.byref(m), mask.ctypes.data_as(_ffi.c_uint8_p))
    assert rc == 0
    out = m.as_dict()
    out["raw"] = bytes(m)
    out["inlier"] = mask[: len(a)]
    return out


def make_matches(seed, n, outlier_share, noise_px=0.3):
    """n matches (pixels) of a camera that drives forward and turns a little, `noise_px` of noise in the second view, a share of
    gross outliers (a point anywhere in the image)."""
    rng = np.random.default_rng(seed)
    yaw, pitch = 0.05 * rng.uniform(-1, 1), 0.01 * rng.uniform(-1, 1)
    cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    R = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    t = np.array([0.1 * rng.uniform(-1, 1), 0.02 * rng.uniform(-1, 1), -1.0])
    X = np.stack([rng.uniform(-10, 10, n), rng.uniform(-2, 2, n), rng.uniform(5, 40, n)], 1)
    Y = X @ R.T + t
    a = FOCAL * X[:, :2] / X[:, 2:3] + (CX, CY)
    b = FOCAL * Y[:, :2] / Y[:, 2:3] + (CX, CY) + noise_px * rng.standard_normal((n, 2))
    out = rng.uniform(0, 1, n) < outlier_share
    b[out] = np.stack([CX + 600 * rng.uniform(-1, 1, n), CY + 180 * rng.uniform(-1, 1, n)], 1)[out]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)
