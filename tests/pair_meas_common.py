"""Test infrastructure of the pair-indexed measurement planes (kba_layout.hpp:BatchView::pair_m): builds and binds the entry
that hands out the packer's planes next to the tables they are built from (tests/cpp/emu_pair_meas.cpp), and holds the window
shapes both tiers run (tests/test_pair_measurements_cpu.py, tests/test_gpu_pair_measurements.py)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

import fixed_lm_common as flc
from limo_amd import _ffi, synth
from limo_amd.window import Window, struct_array

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_BUILD = os.path.join(_HERE, "cpp", "_build")
_CSRC = os.path.join(_ROOT, "limo_amd", "csrc")
LIB = os.path.join(_BUILD, "libkba_emu_pairs.so")
_lib = None

NO_DEPTH, MISSING = np.float32(-1.0), np.float32(-2.0)  # kba_layout.hpp: kPairNoDepth, kPairMissing


def build():
    os.makedirs(_BUILD, exist_ok=True)
    src = [os.path.join(_HERE, "cpp", "emu_pair_meas.cpp"), os.path.join(_CSRC, "kba_pack.cpp")]
    deps = src + [os.path.join(_HERE, "cpp", "emu_pipeline.cpp")] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):  # (tests/emu_ffi.py's flags)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-fPIC", "-shared", "-o", LIB] + src)


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(LIB)
        ip, fp = _ffi.c_int32_p, _ffi.c_float_p
        _lib.emu_pair_planes.argtypes = [C.c_int32, C.POINTER(_ffi.BaWindow), C.POINTER(_ffi.c_uint8_p), C.POINTER(_ffi.BaOptions), C.c_int,
                                         C.POINTER(C.c_int64), ip, fp, fp, fp, fp, fp, fp, ip]
    return _lib


def pair_planes(windows, flag_list, opts, pose_only=False):
    """The batch's lm_slot, its pair planes and its obs_* (as the kernels' view holds them) + per window (lm0, n_lm, n_view, n_view_fixed0)."""
    L = lib()
    arr = struct_array(windows)
    if flag_list is None:
        ptrs, keep = None, None
    else:
        ptrs, keep = flc.flag_pointers([flc.as_flags(f, w.n_lm) for f, w in zip(flag_list, windows)])
    dims = (C.c_int64 * 6)()
    rc = L.emu_pair_planes(len(windows), arr, ptrs, C.byref(opts), int(pose_only), dims, None, None, None, None, None, None, None, None)
    if rc != 0:
        raise RuntimeError("emu_pair_planes rc=%d" % rc)
    vmax, sl, tl, to, n_slot, n_pair = (int(x) for x in dims)
    assert n_slot == n_pair == max(1, vmax) * sl
    slot = np.zeros(n_slot, np.int32)
    pu, pv, pd = (np.zeros(n_slot, np.float32) for _ in range(3))
    ou, ov, od = (np.zeros(max(1, to), np.float32) for _ in range(3))
    win = np.zeros(4 * len(windows), np.int32)
    f = lambda a: a.ctypes.data_as(_ffi.c_float_p)
    i = lambda a: a.ctypes.data_as(_ffi.c_int32_p)
    rc = L.emu_pair_planes(len(windows), arr, ptrs, C.byref(opts), int(pose_only), dims, i(slot), f(pu), f(pv), f(pd), f(ou), f(ov), f(od), i(win))
    if rc != 0:
        raise RuntimeError("emu_pair_planes rc=%d" % rc)
    shp = (max(1, vmax), sl)
    return dict(Vmax=vmax, SL=sl, TL=tl, TO=to, lm_slot=slot.reshape(shp), pair_u=pu.reshape(shp), pair_v=pv.reshape(shp), pair_d=pd.reshape(shp),
                obs_u=ou[:to], obs_v=ov[:to], obs_d=od[:to], win=win.reshape(-1, 4))


# ---- window surgery
def _rebuild(w, lm_keep, obs_keep):
    """The window with the landmarks lm_keep (boolean, caller order kept) and the observations obs_keep of them."""
    obs_keep = obs_keep & lm_keep[w.obs_lm]
    new = -np.ones(w.n_lm, np.int64)
    new[lm_keep] = np.arange(int(lm_keep.sum()))
    d = {name: getattr(w, name).copy() for name, _ in Window.FIELDS}
    for k in ("lm_pos", "lm_weight", "lm_is_ground"):
        d[k] = d[k][lm_keep]
    for k in ("obs_kf", "obs_lm", "obs_cam", "obs_u", "obs_v", "obs_d"):
        d[k] = d[k][obs_keep]
    d["obs_lm"] = new[d["obs_lm"]].astype(np.int32)
    return Window(**d)


def exact(seed, n_lm, **kw):
    """A synth.make_window window of EXACTLY n_lm landmarks (make_window rejects some of those it draws): the first n_lm of a larger draw."""
    w = synth.make_window(seed, n_lm=n_lm + n_lm // 2 + 8, **kw)
    assert w.n_lm >= n_lm
    keep = np.arange(w.n_lm) < n_lm
    return _rebuild(w, keep, np.ones(w.n_obs, bool))


def drop_views(w):
    """Landmark l loses its observation in the FIRST keyframe (l % 4 == 0), in the LAST (l % 4 == 1), or all but one (l % 4 == 2: seen in
    one view only) - never its only one."""
    keep = np.ones(w.n_obs, bool)
    first, last = 0, w.n_kf - 1
    nobs = np.bincount(w.obs_lm, minlength=w.n_lm)
    for o in range(w.n_obs):
        l, k = int(w.obs_lm[o]), int(w.obs_kf[o])
        if nobs[l] < 2:
            continue
        if (l % 4 == 0 and k == first) or (l % 4 == 1 and k == last):
            keep[o] = False
            nobs[l] -= 1
    for l in range(2, w.n_lm, 4):
        obs = np.flatnonzero((w.obs_lm == l) & keep)
        keep[obs[1:]] = False
    return _rebuild(w, np.ones(w.n_lm, bool), keep)


def odd_depths(w, values=(0.0, -1.0, -2.0, -0.5)):
    """Every observation without a depth gets one of the non-positive `values` in turn (the caller's -1 among them)."""
    w = w.copy()
    idx = np.flatnonzero(~(w.obs_d > 0))
    w.obs_d[idx] = np.asarray(values, np.float32)[np.arange(idx.size) % len(values)]
    return w


def shapes():
    """name -> (window, flags or None).  2, 3 and 5 keyframes; 63, 65, 257 and 300 landmarks (one short of a wave, one past it, one past a
    workgroup, a workgroup and a part); two views per keyframe; first / last views missing and landmarks of one view; non-positive caller
    depths; constant landmarks; a window that trims (>= 100 landmarks with the default options: the 257 and 300 ones, and "trim")."""
    out = {}
    out["kf2_63"] = (exact(21, 63, n_kf=2), None)
    out["kf3_65"] = (exact(22, 65, n_kf=3), None)
    out["kf5_257"] = (exact(23, 257, n_kf=5), None)
    out["kf5_300"] = (exact(24, 300, n_kf=5), None)
    out["stereo_130"] = (exact(25, 130, n_kf=3, stereo_baseline=0.5), None)
    out["views_257"] = (drop_views(exact(26, 257, n_kf=5)), None)
    out["views_65"] = (drop_views(exact(27, 65, n_kf=3)), None)
    out["depths_65"] = (odd_depths(exact(28, 65, n_kf=3)), None)
    out["depths_300"] = (odd_depths(exact(29, 300, n_kf=5)), None)
    w = exact(30, 150, n_kf=5)
    out["const_150"] = (w, flc.every(w.n_lm, 3))
    w = drop_views(exact(31, 65, n_kf=4))
    out["const_views_65"] = (w, flc.every(w.n_lm, 2))
    out["trim_400"] = (synth.make_window(32, n_kf=4, n_lm=400, outlier_frac=0.15), None)
    return out


# ---- what a solve of a shape is recorded as (tests/golden/pair_measurements_emu.json)
REPORT_INT = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "num_linearizations", "n_depth_blocks",
              "n_repr_blocks", "n_gp_blocks", "n_trimmed_landmarks")
REPORT_FLOAT = ("initial_cost", "final_cost")
LM_CHUNK = 16  # landmarks per digest of lm_pos: a mismatch names the landmarks it is in


def record(w, rep, trimmed):
    """Counts of the report, its costs and every keyframe parameter as hex floats (a mismatch shows which value moved and by how much),
    the landmarks as one digest per LM_CHUNK of them, the trimmed landmarks."""
    out = {k: int(rep[k]) for k in REPORT_INT}
    out.update({k: float(rep[k]).hex() for k in REPORT_FLOAT})
    for k in ("kf_pose", "kf_plane_dir", "kf_plane_dist"):
        out[k] = [float(x).hex() for x in np.asarray(getattr(w, k)).ravel()]
    out["lm_pos"] = [hashlib.sha256(w.lm_pos[i:i + LM_CHUNK].tobytes()).hexdigest()[:16] for i in range(0, w.n_lm, LM_CHUNK)]
    out["trimmed"] = [int(i) for i in trimmed]
    return out


def first_difference(got, want):
    """Where two records part: the first key, and inside a list the first index."""
    for k in sorted(want):
        if got.get(k) != want[k]:
            if isinstance(want[k], list) and isinstance(got.get(k), list) and len(got[k]) == len(want[k]):
                i = next(i for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b)
                return "%s[%d]: %s, golden %s" % (k, i, got[k][i], want[k][i])
            return "%s: %s, golden %s" % (k, got.get(k), want[k])
    return None


def solve_all(opts, n_slots=0):
    """name -> record of the shape solved by the emulated pipeline as a batch of one (n_slots > 0: the streaming schedule)."""
    out = {}
    for name, (w, flags) in sorted(shapes().items()):
        ws = [w.copy()]
        reps, trimmed = flc.emu_solve_batch(ws, None if flags is None else [flags], opts, n_slots)
        out[name] = record(ws[0], reps[0], trimmed[0])
    return out
