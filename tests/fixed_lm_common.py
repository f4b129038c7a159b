"""Test infrastructure of the fixed-landmark solve: builds and binds its checker (tests/cpp/fixed_lm_ref.cpp: the oracle with
the flagged landmarks set constant) and the emulated pipeline with a flags entry (tests/cpp/emu_fixed_lm.cpp), and holds the
window shapes both tiers run (tests/test_fixed_landmarks_cpu.py, tests/test_gpu_fixed_landmarks.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from limo_amd import _ffi, synth
from limo_amd.window import struct_array

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_BUILD = os.path.join(_HERE, "cpp", "_build")
REF_LIB = os.path.join(_BUILD, "libfixed_lm_ref.so")
EMU_LIB = os.path.join(_BUILD, "libkba_emu_fixed.so")
_CSRC = os.path.join(_ROOT, "limo_amd", "csrc")
_ref = _emu = None


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def build():
    os.makedirs(_BUILD, exist_ok=True)
    odir = os.path.join(_ROOT, "oracle")
    ref_src = [os.path.join(_HERE, "cpp", "fixed_lm_ref.cpp"), os.path.join(odir, "ceres_like.cpp")]
    if _stale(REF_LIB, ref_src + [os.path.join(odir, f) for f in ("kba_oracle.cpp", "ceres_like.hpp", "functors.hpp", "jet.hpp")]):
        # (oracle/Makefile's flags: the checker computes what liboracle.so computes)
        subprocess.check_call(["g++", "-O3", "-march=x86-64-v4", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", REF_LIB] + ref_src)
    emu_src = [os.path.join(_HERE, "cpp", "emu_fixed_lm.cpp"), os.path.join(_CSRC, "kba_pack.cpp")]
    deps = emu_src + [os.path.join(_HERE, "cpp", "emu_pipeline.cpp")] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if _stale(EMU_LIB, deps):  # (tests/emu_ffi.py's flags)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-fPIC", "-shared", "-o", EMU_LIB] + emu_src)


def _u8(a):
    return None if a is None else a.ctypes.data_as(_ffi.c_uint8_p)


def ref():
    global _ref
    if _ref is None:
        build()
        _ref = C.CDLL(REF_LIB)
        _ref.ref_ba_solve_fixed.argtypes = [C.POINTER(_ffi.BaWindow), _ffi.c_uint8_p, C.POINTER(_ffi.BaOptions), C.POINTER(_ffi.BaReport)]
        _ref.ref_last_trimmed.argtypes = [_ffi.c_int32_p, C.c_int]
        _ref.ref_set_threads.argtypes = [C.c_int]
        _ref.ref_set_threads.restype = None
    return _ref


def emu():
    global _emu
    if _emu is None:
        build()
        _emu = C.CDLL(EMU_LIB)
        _emu.emu_ba_solve_batch_fixed.argtypes = [C.c_int32, C.POINTER(_ffi.BaWindow), C.POINTER(_ffi.c_uint8_p), C.POINTER(_ffi.BaOptions), C.POINTER(_ffi.BaReport), C.c_int]
        _emu.emu_last_trimmed.argtypes = [C.c_int, _ffi.c_int32_p, C.c_int]
        ip = _ffi.c_int32_p
        _emu.emu_pack_layout.argtypes = [C.POINTER(_ffi.BaWindow), _ffi.c_uint8_p, C.POINTER(_ffi.BaOptions), ip, ip, _ffi.c_uint8_p, ip, C.c_int32, ip, ip]
        _emu.emu_pack_equal.argtypes = [C.c_int32, C.POINTER(_ffi.BaWindow), C.POINTER(_ffi.c_uint8_p), C.POINTER(_ffi.BaOptions)]
    return _emu


def as_flags(flags, n_lm):
    """uint8 array of n_lm flags (at least one byte long), or None."""
    if flags is None:
        return None
    f = np.ascontiguousarray(np.asarray(flags).astype(bool).astype(np.uint8))
    assert f.size == n_lm
    return f if n_lm else np.zeros(1, np.uint8)


def flag_pointers(flag_list):
    keep = list(flag_list)
    return (_ffi.c_uint8_p * max(1, len(keep)))(*[_u8(f) for f in keep]), keep


def ref_solve(window, flags, opts, threads=1):
    """The checker on `window` IN PLACE.  Returns (report dict, sorted trimmed landmark indices)."""
    lib = ref()
    lib.ref_set_threads(int(threads))
    s = window.as_struct()
    rep = _ffi.BaReport()
    rc = lib.ref_ba_solve_fixed(C.byref(s), _u8(as_flags(flags, window.n_lm)), C.byref(opts), C.byref(rep))
    if rc != 0:
        raise RuntimeError("ref_ba_solve_fixed rc=%d" % rc)
    n = lib.ref_last_trimmed(None, 0)
    out = np.zeros(max(1, n), np.int32)
    lib.ref_last_trimmed(out.ctypes.data_as(_ffi.c_int32_p), n)
    return rep.as_dict(), np.sort(out[:n])


def emu_solve_batch(windows, flag_list, opts, n_slots=0):
    """The emulated pipeline on `windows` IN PLACE (flag_list: None, or one entry per window, each None or flags).  n_slots > 0:
    the streaming schedule.  Returns (reports, trimmed index arrays)."""
    lib = emu()
    arr = struct_array(windows)
    reps = (_ffi.BaReport * len(windows))()
    if flag_list is None:
        ptrs, keep = None, None
    else:
        ptrs, keep = flag_pointers([as_flags(f, w.n_lm) for f, w in zip(flag_list, windows)])
    rc = lib.emu_ba_solve_batch_fixed(len(windows), arr, ptrs, C.byref(opts), reps, int(n_slots))
    if rc != 0:
        raise RuntimeError("emu_ba_solve_batch_fixed rc=%d" % rc)
    trimmed = []
    for i in range(len(windows)):
        n = lib.emu_last_trimmed(i, None, 0)
        out = np.zeros(max(1, n), np.int32)
        lib.emu_last_trimmed(i, out.ctypes.data_as(_ffi.c_int32_p), n)
        trimmed.append(np.sort(out[:n]))
    return [r.as_dict() for r in reps], trimmed


def pack_layout(window, flags, opts, cap=256):
    """The packed layout of one window: dict of the descriptor's counts and the per-landmark / per-block tables."""
    lib = emu()
    s = window.as_struct()
    n = window.n_lm
    counts = np.zeros(8, np.int32)
    lm_id, lm_gp, lm_state = np.zeros(max(1, n), np.int32), np.zeros(max(1, n), np.int32), np.zeros(max(1, n), np.uint8)
    lblk, sblk = np.zeros(2 * cap, np.int32), np.zeros(2 * cap, np.int32)
    ip = lambda a: a.ctypes.data_as(_ffi.c_int32_p)
    rc = lib.emu_pack_layout(C.byref(s), _u8(as_flags(flags, n)), C.byref(opts), ip(counts), ip(lm_id), _u8(lm_state), ip(lm_gp), cap, ip(lblk), ip(sblk))
    if rc != 0:
        raise RuntimeError("emu_pack_layout rc=%d" % rc)
    keys = ("n_lm_const", "n_lblk", "n_sblk", "n_sblk_plain", "lm_gp0", "n_gp", "n_view_fixed0", "nf")
    out = dict(zip(keys, (int(v) for v in counts)))
    assert out["n_lblk"] <= cap and out["n_sblk"] <= cap
    out.update(lm_id=lm_id[:n], lm_state=lm_state[:n], lm_gp=lm_gp[:n], lblk=lblk[: 2 * out["n_lblk"]].reshape(-1, 2), sblk=sblk[: 2 * out["n_sblk"]].reshape(-1, 2))
    return out


def pack_equal(windows, flag_list, opts):
    lib = emu()
    arr = struct_array(windows)
    ptrs, keep = flag_pointers([as_flags(f, w.n_lm) for f, w in zip(flag_list, windows)])
    return lib.emu_pack_equal(len(windows), arr, ptrs, C.byref(opts))


# ---- the shapes of both tiers: name -> (window, flags)
def every(n_lm, m):
    return (np.arange(n_lm) % m == 0).astype(np.uint8)


def shapes():
    """(a) - (e) of the feature's issue, then (f), then (g) = (a) - (e) with every keyframe's fixation LIMO_FIX_NONE, then (h) =
    some of them with pose-fixed keyframes in the middle or at the end of the window."""
    out = {}
    w = synth.make_window(8, n_kf=2, n_lm=12)
    out["a"] = (w, every(w.n_lm, 3))
    w = synth.make_window(7, n_kf=3, n_lm=33)
    out["b"] = (w, ((w.lm_is_ground != 0) | (every(w.n_lm, 3) != 0)).astype(np.uint8))
    w = synth.make_window(2, n_kf=4, n_lm=150)
    out["c2"] = (w, every(w.n_lm, 2))
    w = synth.make_window(3, n_kf=5, n_lm=300)
    out["c3"] = (w, every(w.n_lm, 3))
    w = synth.make_window(5, n_kf=4, n_lm=150, with_ground_plane=False)
    out["d"] = (w, every(w.n_lm, 3))
    w = synth.make_window(6, n_kf=5, n_lm=400, stereo_baseline=0.5)
    out["e3"] = (w, every(w.n_lm, 3))
    out["e_all"] = (w.copy(), np.ones(w.n_lm, np.uint8))
    w = out["a"][0].copy()
    w.kf_fixation[:] = _ffi.LIMO_FIX_POSE
    out["f"] = (w, np.ones(w.n_lm, np.uint8))
    for k in ("a", "b", "c2", "c3", "d", "e3", "e_all"):
        w = out[k][0].copy()
        w.kf_fixation[:] = _ffi.LIMO_FIX_NONE
        out["g_" + k] = (w, out[k][1])
    # (h) LIMO_FIX_POSE keyframes that do not lead the window: the fixed-cost rule holds for any kf_fixation pattern
    P, N = _ffi.LIMO_FIX_POSE, _ffi.LIMO_FIX_NONE
    for name, k, fix in (("h_e_all_02", "e_all", [P, N, P, N, N]), ("h_e_all_1", "e_all", [N, P, N, N, N]), ("h_b_02", "b", [P, N, P]),
                         ("h_e3_024", "e3", [P, N, P, N, P]), ("h_d_3", "d", [N, N, N, P])):
        w = out[k][0].copy()
        w.kf_fixation[:] = fix
        out[name] = (w, out[k][1])
    return out


def sweep(n=48, seed=4242):
    """The mixed sweep: fuzz_common.random_windows with a flag density of 0.1 / 0.5 / 1.0 drawn per window, or no flags at all."""
    import fuzz_common as fc

    rng = np.random.default_rng(seed + 1)
    out = []
    for kw, w in fc.random_windows(n, seed):
        dens = rng.choice([-1.0, 0.1, 0.5, 1.0])
        flags = None if dens < 0 else (np.ones(w.n_lm, np.uint8) if dens == 1.0 else (rng.random(w.n_lm) < dens).astype(np.uint8))
        out.append((kw, w, flags))
    return out


def check_parity(w, rep_x, end_x, trimmed_x, solve_x, rep_o, end_o, trimmed_o, solve_o):
    """fuzz_common.check_parity, for windows WITH or WITHOUT a LIMO_FIX_POSE keyframe 0.  The rule has a clause of its
    own for the pose-fixed keyframe 0 of a sliding window ("Pose-fixed keyframe moved"), which says nothing about a window whose
    keyframe 0 is free.  Such a window has to be well posed and to meet the STRICT clause - 1e-4 on every keyframe translation,
    keyframe 0 included, and on the cost; same termination; the rule's counts and trimmed sets - and nothing weaker: the rule is
    handed the solved keyframe 0 as the input's, which the STRICT clause uses for nothing but the clause that does not apply."""
    import fuzz_common as fc

    if w.kf_fixation[0] == _ffi.LIMO_FIX_POSE:
        return fc.check_parity(w, rep_x, end_x, trimmed_x, solve_x, rep_o, end_o, trimmed_o, solve_o)
    if not fc.well_posed(w):
        return False, "a window without a pose-fixed keyframe 0 has to be well posed: the rule's weak checks are not defined for it", False
    ep, ec = fc.rel_pose_err(end_x.kf_pose, end_o.kf_pose), fc.rel_cost_err(rep_x, rep_o)
    if not (ep <= fc.TOL and ec <= fc.TOL and rep_x["termination"] == rep_o["termination"]):
        return False, "a window without a pose-fixed keyframe 0 has to meet the strict clause: pose %.2e cost %.2e terminations %r / %r" % (
            ep, ec, rep_x["termination"], rep_o["termination"]), False
    w0 = w.copy()
    w0.kf_pose[0] = end_x.kf_pose[0]
    ok, detail, clause = fc.check_parity(w0, rep_x, end_x, trimmed_x, solve_x, rep_o, end_o, trimmed_o, solve_o)
    return ok and clause == fc.STRICT, detail, clause
