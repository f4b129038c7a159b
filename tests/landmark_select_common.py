"""Test infrastructure of the device landmark selection (include/limo_hip.h:limo_landmark_select), shared by the CPU tier
(tests/test_landmark_select_cpu.py), the GPU tier (tests/test_gpu_landmark_select.py) and scripts/bench_landmark_select.py: the checker
library (tests/cpp/landmark_select_ref.cpp: Keyframe / Landmark objects and LandmarkSelector with cheirality + voxel + add-depth as
StreamDriver wires them, compiled with -ffp-contract=off), the stand-alone test of limo_amd/csrc/landmark_select_core.hpp
(tests/cpp/test_landmark_select_core.cpp, plain and under the sanitizers) and the seeded pool generator."""
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
REF_LIB = os.path.join(_BUILD, "libselect_ref.so")
UNIT = os.path.join(_BUILD, "test_landmark_select_core")
UNIT_SAN = os.path.join(_BUILD, "test_landmark_select_core_san")
FOCAL, CX, CY = 718.856, 607.1928, 185.2157  # KITTI 00
_ref = None


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _headers():
    return [os.path.join(_CSRC, f) for f in ("landmark_select_core.hpp", "kba_math.hpp")] + \
        [os.path.join(_KBA, f) for f in ("landmark_selector.hpp", "landmark_selection_voxel.hpp", "keyframe.hpp", "definitions.hpp")] + \
        [os.path.join(_ROOT, "include", "limo_hip.h"), os.path.join(_HERE, "cpp", "landmark_select_ref.cpp")]


def build_unit():
    """tests/cpp/test_landmark_select_core.cpp, plain and under -fsanitize=address,undefined (a stand-alone host program)."""
    os.makedirs(_BUILD, exist_ok=True)
    src = os.path.join(_HERE, "cpp", "test_landmark_select_core.cpp")
    if _stale(UNIT, [src] + _headers()):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-o", UNIT, src])
    if _stale(UNIT_SAN, [src] + _headers()):
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                               "-ffp-contract=off", "-std=c++17", "-o", UNIT_SAN, src])
    return UNIT, UNIT_SAN


def build():
    os.makedirs(_BUILD, exist_ok=True)
    src = os.path.join(_HERE, "cpp", "landmark_select_ref.cpp")
    if _stale(REF_LIB, [src] + _headers()):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-o", REF_LIB, src])
    build_unit()


def ref_lib():
    global _ref
    if _ref is None:
        build()
        _ref = C.CDLL(REF_LIB)
        _ref.landmark_select_ref.argtypes = [C.POINTER(_ffi.SelectPool), C.POINTER(_ffi.SelectParams), _ffi.c_uint8_p, _ffi.c_double_p, C.c_int32]
    return _ref


def params(add=(), **fields):
    """struct limo_select_params: the node's values (limo_select_default_params) with the given fields replaced, and a must-have list.
    Needs no device and no liblimo_hip.so."""
    p = _ffi.SelectParams()
    p.voxel_size_xyz[:] = [0.5, 0.5, 0.3]
    p.roi_far, p.roi_middle, p.max_near, p.max_middle, p.max_far = 40.0, 15.0, 200, 200, 100
    for name, v in fields.items():
        if name == "voxel_size_xyz":
            p.voxel_size_xyz[:] = [float(x) for x in v]
        else:
            setattr(p, name, v)
    if len(add):
        p._add_keep = (_ffi.SelectAdd * len(add))(*[_ffi.SelectAdd(*(int(x) for x in a)) for a in add])
        p.add, p.n_add = p._add_keep, len(add)
    return p


def with_fields(p, **fields):
    """A copy of a params struct (the must-have list shared) with fields replaced."""
    q = _ffi.SelectParams.from_buffer_copy(p)
    q._add_keep = getattr(p, "_add_keep", None)
    for name, v in fields.items():
        if name == "voxel_size_xyz":
            q.voxel_size_xyz[:] = [float(x) for x in v]
        else:
            setattr(q, name, v)
    return q


def ref_select(pool, p, seconds=None, no_cheirality=False):
    """The host classes on the pool: one byte per landmark, as limo_landmark_select documents it."""
    w, keep = _ffi.select_pool(pool)
    out = np.zeros(max(1, w.n_lm), np.uint8)
    sec = C.c_double(0.0)
    rc = ref_lib().landmark_select_ref(C.byref(w), C.byref(p), out.ctypes.data_as(_ffi.c_uint8_p), C.byref(sec), 1 if no_cheirality else 0)
    assert rc == 0, rc
    if seconds is not None:
        seconds.append(sec.value)
    del keep
    return out[: w.n_lm]


def quat_R(q):
    """kba_math.hpp:quat_R (the polynomial rotation, not normalised)."""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# the node's must-have wiring in small (sequence.hpp: configureSequence): the nearest landmarks with a measured depth in the oldest keyframe, the
# nearest ground landmarks of the first four keyframes of the window
ADD = [(0, 5, _ffi.SELECT_HAS_DEPTH, _ffi.SELECT_KEY_MEASURED_DEPTH)] + [(i, 6, _ffi.SELECT_IS_GROUND, _ffi.SELECT_KEY_RANGE) for i in range(4)]


def make_pool(seed, n_lm, n_kf, n_cam=1, straight=False, behind_share=0.03, double_share=0.3, unseen_share=0.05, cam1_tz=0.0, equal_flow=False):
    """A KITTI-shaped window: the vehicle (= camera 0 frame, z forward, y down) drives ~1.2 m per keyframe with a little yaw; landmarks lie
    in the frustum of the newest keyframe out to 115 m, 20 % of them on the ground, some next to the landmark before them (shared voxels),
    some behind the older keyframes (cheirality); float measurements, some with a depth.  Observations in (kf, lm, cam) order.
      straight      no rotation, no lateral motion (the newest keyframe's frame is the world shifted)
      equal_flow    every landmark measured by every keyframe and camera at the same pixel per keyframe: equal flows, equal track lengths"""
    rng = np.random.default_rng(seed)
    kf_pose = np.zeros((n_kf, 7))
    centres = np.zeros((n_kf, 3))
    z = 0.0
    for k in range(n_kf):
        yaw = 0.0 if straight else 0.015 * k + 0.005 * rng.uniform(-1, 1)
        q = np.array([np.cos(yaw / 2), 0.0, np.sin(yaw / 2), 0.0])
        c = np.array([0.0 if straight else 0.2 * rng.uniform(-1, 1), 0.0, z])
        z += rng.uniform(0.9, 1.5)
        kf_pose[k, :4], kf_pose[k, 4:], centres[k] = q, -quat_R(q) @ c, c
    kf_stamp = (1_000_000_000 + 100_000_000 * np.arange(n_kf)).astype(np.uint64)
    cam = np.array([[FOCAL, CX, CY, 1, 0, 0, 0, -0.54 * c, 0, cam1_tz if c else 0.0] for c in range(n_cam)], np.float64).reshape(n_cam, 10)
    z_new = centres[-1, 2] if n_kf else 0.0
    z_old = centres[0, 2] if n_kf else 0.0
    lm_pos = np.zeros((n_lm, 3))
    lm_is_ground = rng.uniform(0, 1, n_lm) < 0.2
    for i in range(n_lm):
        u = rng.uniform(0, 1)
        if i > 0 and u < double_share:
            lm_pos[i] = lm_pos[i - 1] + 0.12 * rng.uniform(-1, 1, 3)
            lm_is_ground[i] = lm_is_ground[i - 1]
            continue
        depth = rng.uniform(2, 115) if u > double_share + behind_share else rng.uniform(-5, 0.5) - (z_new - z_old)
        lat = rng.uniform(-1, 1) * (0.5 * abs(depth) + 2)
        lm_pos[i] = (lat, 1.65 if lm_is_ground[i] else rng.uniform(-3, 1.5), z_new + depth)
    lm_id = np.cumsum(rng.integers(1, 4, n_lm)).astype(np.uint64) + 100
    lm_has_depth = rng.uniform(0, 1, n_lm) < 0.4
    # measured in keyframes [k0, k1): most tracks live on to the newest keyframe, a few are measured nowhere; camera 1 sees 70 %
    k0 = np.zeros(n_lm, np.int64) if equal_flow or n_kf == 0 else rng.integers(0, n_kf, n_lm)
    k1 = np.where(rng.uniform(0, 1, n_lm) < 0.8, n_kf, k0 + (rng.uniform(0, 1, n_lm) * (n_kf - k0 + 1)).astype(np.int64))
    k1 = np.where(rng.uniform(0, 1, n_lm) < unseen_share, k0, k1)
    if equal_flow:
        k1[:] = n_kf
    kk = np.arange(n_kf)
    seen = (kk[None, :, None] >= k0[:, None, None]) & (kk[None, :, None] < k1[:, None, None]) & np.ones((1, 1, n_cam), bool)
    if not equal_flow:
        seen[:, :, 1:] &= rng.uniform(0, 1, (n_lm, n_kf, max(0, n_cam - 1))) >= 0.3
    R = np.array([quat_R(q[:4]) for q in kf_pose]).reshape(n_kf, 3, 3)
    with np.errstate(all="ignore"):
        Y = np.einsum("kab,ib->ika", R, lm_pos) + kf_pose[None, :, 4:]  # [lm, kf, 3] in the vehicle frame
        zc = Y[:, :, 2:3] + np.array([cam1_tz if c else 0.0 for c in range(n_cam)])[None, None, :]
        zs = np.where(np.abs(zc) > 0.1, zc, 0.1)
        u = FOCAL * (Y[:, :, 0:1] - 0.54 * np.arange(n_cam)[None, None, :]) / zs + CX + 0.3 * rng.standard_normal((n_lm, n_kf, n_cam))
        v = FOCAL * Y[:, :, 1:2] / zs + CY + 0.3 * rng.standard_normal((n_lm, n_kf, n_cam))
    if equal_flow:
        u = np.broadcast_to((100.0 + 7 * kk)[None, :, None], u.shape)
        v = np.broadcast_to((50.0 + 3 * kk)[None, :, None], v.shape)
    d = np.where(lm_has_depth[:, None, None] & (rng.uniform(0, 1, (n_lm, n_kf, n_cam)) < 0.7), zc, -1.0)
    oi, ok, oc = np.nonzero(seen)
    order = np.lexsort((oc, oi, ok))  # (kf, lm, cam) order
    oi, ok, oc = oi[order], ok[order], oc[order]
    o = np.stack([ok, oi, oc, u[oi, ok, oc], v[oi, ok, oc], d[oi, ok, oc]], 1).astype(np.float64).reshape(-1, 6)
    return {"kf_pose": kf_pose, "kf_stamp": kf_stamp, "cam": cam, "lm_id": lm_id, "lm_pos": lm_pos, "lm_has_depth": lm_has_depth.astype(np.uint8),
            "lm_is_ground": lm_is_ground.astype(np.uint8), "obs_kf": o[:, 0].astype(np.int32), "obs_lm": o[:, 1].astype(np.int32), "obs_cam": o[:, 2].astype(np.int32),
            "obs_u": o[:, 3].astype(np.float32), "obs_v": o[:, 4].astype(np.float32), "obs_d": o[:, 5].astype(np.float32), "centres": centres}


def shuffled(pool, seed):
    """The same pool with its observations in another order."""
    perm = np.random.default_rng(seed).permutation(len(pool["obs_kf"]))
    out = dict(pool)
    for k in ("obs_kf", "obs_lm", "obs_cam", "obs_u", "obs_v", "obs_d"):
        out[k] = pool[k][perm]
    return out


def voxel_sizes(pool, p, keep):
    """Member counts of the occupied voxels (numpy arithmetic: statistics of a test pool, not a checker) among the landmarks `keep`
    (boolean: those the checker did not reject)."""
    n_kf = len(pool["kf_stamp"])
    if n_kf == 0 or not keep.any():
        return np.zeros(0, np.int64)
    new = int(np.argmax(pool["kf_stamp"]))
    R, t = quat_R(pool["kf_pose"][new, :4]), pool["kf_pose"][new, 4:]
    P = pool["lm_pos"][keep] @ R.T + t
    path = np.array([R @ (-quat_R(q[:4]).T @ q[4:]) + t for q in pool["kf_pose"]])
    with np.errstate(all="ignore"):
        if n_kf == 1:
            d = np.linalg.norm(P - path[0], axis=1)
        else:
            d = np.full(len(P), np.inf)
            for a, b in zip(path[:-1], path[1:]):
                ab = b - a
                l2 = ab @ ab
                s = np.clip(((P - a) @ ab) / l2, 0, 1) if l2 > 0 else np.zeros(len(P))
                d = np.fmin(d, np.linalg.norm(P - (a + s[:, None] * ab), axis=1))
        pipe = (P[:, 2] >= -20) & (P[:, 2] <= 100) & (d < p.roi_far)
        cells = np.floor(P[pipe] / np.array(p.voxel_size_xyz[:]))
    if len(cells) == 0:
        return np.zeros(0, np.int64)
    return np.unique(cells, axis=0, return_counts=True)[1]
