"""The marginal pose covariance of a solved window (include/limo_hip.h, "Pose covariance") held to a dense reference, shared by the
CPU tier (tests/test_pose_covariance_cpu.py: the emulator running kba_items.hpp:cam_cov) and the GPU tier
(tests/test_gpu_pose_covariance.py: k_cam_cov behind every launch path).

REFERENCE.  Plain numpy on lm_step_common.Linearisation(w0, opts, at=<the implementation's final window>, problem=...): `Ju` and `col`
are the dense unscaled tangent Jacobian of the problem built at w0, robustified, at the final point.  For a trimmed solve the columns
of the trimmed landmarks go, and every row with a non-zero in them (asserted to be the observation rows of those landmarks plus at
most one ground-plane row per trimmed ground landmark, so the rule cannot silently miss).  The three columns of every free plane
normal are expressed in a minimal basis (two columns orthogonal to n), J = Q R, and the covariance is R^-1 R^-T; its pose rows and
columns, at 6 k + component for keyframe k, are what the implementation's matrix is compared with: every free keyframe's 6 x 6
diagonal block ("block") and the whole pose matrix ("full") in relative Frobenius norm.

BARS.  The rule of lm_step_common.py, one bar per class: 100 x the largest deviation of the emulator from this reference over all
CPU cases, rounded up to one digit; the CPU tier measures the spread again on every run and fails when it has outgrown a bar's
hundredth by more than a factor of two.  A case that would need a bar above 1e-6 is ill-conditioned input (every regular shape has
cond(R) <= 1.3e8): its seed is replaced, the bar is not widened.  Never derived from the GPU, whose own maxima are recorded in
profiles/pose_covariance.md.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import fixed_lm_common as flc
import lm_step_common as lsc
import pyoracle
from limo_amd import _ffi, default_options
from limo_amd.window import struct_array

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_BUILD = os.path.join(_HERE, "cpp", "_build")
_CSRC = os.path.join(_ROOT, "limo_amd", "csrc")
EMU_LIB = os.path.join(_BUILD, "libkba_emu_cov.so")
UNIT = os.path.join(_BUILD, "test_pose_cov")
UNIT_SAN = os.path.join(_BUILD, "test_pose_cov_san")
_emu = None

OK, RANK_DEFICIENT, NO_FREE_POSE, EVAL_FAILED, NOT_COMPUTED = (_ffi.LIMO_COV_OK, _ffi.LIMO_COV_RANK_DEFICIENT, _ffi.LIMO_COV_NO_FREE_POSE,
                                                                _ffi.LIMO_COV_EVAL_FAILED, _ffi.LIMO_COV_NOT_COMPUTED)

# measured CPU spread x 100, rounded up to one digit (test_pose_covariance_cpu.py::test_bars_are_100x_the_cpu_spread)
BARS = {
    "block": 2e-11,  # CPU spread 1.93e-13 (shape 7401)
    "full": 2e-11,   # 1.93e-13 (shape 7401: one free keyframe, the block is the matrix)
}
MAX_BAR = 1e-6


# ------------------------------------------------------------------------------------------------ build
def _headers():
    return [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")] + [os.path.join(_ROOT, "include", "limo_hip.h")]


def build():
    """The emulator entry (tests/cpp/emu_pose_cov.cpp, with tests/emu_ffi.py's flags) and the stand-alone host check
    (tests/cpp/test_pose_cov.cpp), plain and under -fsanitize=address,undefined."""
    os.makedirs(_BUILD, exist_ok=True)
    emu_src = [os.path.join(_HERE, "cpp", "emu_pose_cov.cpp"), os.path.join(_CSRC, "kba_pack.cpp")]
    if flc._stale(EMU_LIB, emu_src + [os.path.join(_HERE, "cpp", "emu_pipeline.cpp")] + _headers()):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-fPIC", "-shared", "-o", EMU_LIB] + emu_src)
    src = os.path.join(_HERE, "cpp", "test_pose_cov.cpp")
    if flc._stale(UNIT, [src] + _headers()):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-o", UNIT, src])
    if flc._stale(UNIT_SAN, [src] + _headers()):
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                               "-ffp-contract=off", "-std=c++17", "-o", UNIT_SAN, src])
    return UNIT, UNIT_SAN


def emu():
    global _emu
    if _emu is None:
        build()
        _emu = C.CDLL(EMU_LIB)
        _emu.emu_ba_solve_batch_cov.argtypes = [C.c_int32, C.POINTER(_ffi.BaWindow), C.POINTER(_ffi.c_uint8_p), C.POINTER(_ffi.BaOptions), C.POINTER(_ffi.BaReport),
                                                C.c_int, C.POINTER(_ffi.SpeedPrior), C.c_int, _ffi.c_double_p, _ffi.c_int32_p]
        _emu.emu_last_trimmed.argtypes = [C.c_int, _ffi.c_int32_p, C.c_int]
    return _emu


def emu_solve(windows, opts, problem=lsc.SOLVE, n_slots=0):
    """The emulated pipeline and the covariance pass on `windows` IN PLACE (all of the kind `problem`).
    Returns (reports, [matrix 6 n_kf x 6 n_kf], [status], [trimmed landmark indices])."""
    lib = emu()
    arr = struct_array(windows)
    n = len(windows)
    reps = (_ffi.BaReport * n)()
    sizes = [36 * w.n_kf * w.n_kf for w in windows]
    cov = np.full(sum(sizes), -7.0)
    status = np.full(n, -1, np.int32)
    ptrs, keep = None, None
    if problem.lm_fixed is not None:
        keep = [problem.flags(w.n_lm) for w in windows]
        ptrs = (_ffi.c_uint8_p * n)(*[f.ctypes.data_as(_ffi.c_uint8_p) for f in keep])
    rc = lib.emu_ba_solve_batch_cov(n, arr, ptrs, C.byref(opts), reps, int(problem.pose_only), None if problem.prior is None else C.byref(problem.prior), int(n_slots),
                                    cov.ctypes.data_as(_ffi.c_double_p), status.ctypes.data_as(_ffi.c_int32_p))
    if rc != 0:
        raise RuntimeError("emu_ba_solve_batch_cov rc=%d" % rc)
    mats, off, trimmed = [], 0, []
    for i, w in enumerate(windows):
        mats.append(cov[off : off + sizes[i]].reshape(6 * w.n_kf, 6 * w.n_kf).copy())
        off += sizes[i]
        buf = np.zeros(max(1, w.n_lm), np.int32)
        k = lib.emu_last_trimmed(i, buf.ctypes.data_as(_ffi.c_int32_p), buf.size)
        trimmed.append(np.sort(buf[: max(0, k)].copy()))
    return [r.as_dict() for r in reps], mats, [int(s) for s in status], trimmed


# ------------------------------------------------------------------------------------------------ the reference
class Reference:
    """The reference covariance of the solve of `w0` under `opts` that ended at `final` with the landmarks `trimmed` removed.
    rank_deficient: R has a diagonal entry below 1e-10 of its largest (the free gauge of shape 7306 gives 1e-16); cov is None then.
    free: the keyframes with a free pose block.  The keyword arguments build the deliberately WRONG references of the sensitivity
    tests: damping (radius, options) left on, the Jacobi scale not undone."""

    def __init__(self, w0, final, opts, problem=lsc.SOLVE, trimmed=(), damping=None, keep_scale=False):
        lin = lsc.Linearisation(w0, opts, at=final, problem=problem)
        J, col = lin.Ju, lin.col
        trimmed = [int(t) for t in trimmed]
        self.n_rows_removed = 0
        if trimmed:
            gone = np.array([k == pyoracle.COL_LANDMARK and i in set(trimmed) for k, i, _ in col])
            rows = np.abs(J[:, gone]).sum(1) != 0.0
            sel = np.isin(w0.obs_lm, trimmed)
            rows_obs = int((2 + (w0.obs_d[sel] > 0)).sum())
            n_ground = int((w0.lm_is_ground[trimmed] != 0).sum())
            self.n_rows_removed, self.rows_obs = int(rows.sum()), rows_obs
            assert rows_obs <= rows.sum() <= rows_obs + n_ground, (rows_obs, int(rows.sum()), n_ground)
            J, col = J[~rows][:, ~gone], col[~gone]
        n_kf = w0.n_kf
        # minimal basis of every free plane normal
        cols, pose_of = [], {}
        normals = sorted({int(i) for k, i, _ in col if k == pyoracle.COL_PLANE_DIR})
        done = set()
        for j, (k, i, c) in enumerate(col):
            if k == pyoracle.COL_PLANE_DIR:
                if int(i) in done:
                    continue
                done.add(int(i))
                idx = [jj for jj, (kk, ii, _) in enumerate(col) if kk == k and ii == i]
                assert [int(col[jj][2]) for jj in idx] == [0, 1, 2]
                n = final.kf_plane_dir[int(i)] / np.linalg.norm(final.kf_plane_dir[int(i)])
                B = np.linalg.svd(np.eye(3) - np.outer(n, n))[0][:, :2]
                cols.extend((J[:, idx] @ B).T)
            else:
                if k == pyoracle.COL_POSE:
                    pose_of[len(cols)] = 6 * int(i) + int(c)
                cols.append(J[:, j])
        Jm = np.array(cols).T
        self.n_normals = len(normals)
        self.free = sorted({r // 6 for r in pose_of.values()})
        scale = 1.0 / (1.0 + np.sqrt((Jm**2).sum(0)))  # Ceres' Jacobi scale of these columns
        self.pose_scale = np.zeros(6 * n_kf)
        for j, r in pose_of.items():
            self.pose_scale[r] = scale[j]
        if damping is not None:  # (wrong on purpose) the damped system of a step at `radius`: D^2 = clamp(diag) / radius in the scaled system
            radius, o = damping
            Js = Jm * scale
            D = np.sqrt(np.clip((Js**2).sum(0), o.min_lm_diagonal, o.max_lm_diagonal) / radius)
            Jm = np.vstack([Js, np.diag(D)]) / scale
        R = np.linalg.qr(Jm, mode="r")
        d = np.abs(np.diag(R))
        self.cond = float(np.linalg.cond(R)) if d.min() > 0 else float("inf")
        self.rank_deficient = Jm.shape[0] < Jm.shape[1] or bool(d.min() <= 1e-10 * d.max())
        self.cov = None
        if self.rank_deficient:
            return
        Ri = np.linalg.solve(R, np.eye(R.shape[0]))
        full = Ri @ Ri.T
        self.cov = np.zeros((6 * n_kf, 6 * n_kf))
        js = sorted(pose_of)
        rs = [pose_of[j] for j in js]
        self.cov[np.ix_(rs, rs)] = full[np.ix_(js, js)]
        if keep_scale:  # (wrong on purpose) the covariance of the scaled variables
            s = np.where(self.pose_scale > 0, self.pose_scale, 1.0)
            self.cov = self.cov / np.outer(s, s)


def deviation(got, ref_cov, free):
    """{"block": the largest relative Frobenius deviation of a free keyframe's 6 x 6 diagonal block, "full": that of the whole matrix}"""
    out = {"block": 0.0, "full": float(np.linalg.norm(got - ref_cov) / np.linalg.norm(ref_cov))}
    for k in free:
        s = slice(6 * k, 6 * k + 6)
        out["block"] = max(out["block"], float(np.linalg.norm(got[s, s] - ref_cov[s, s]) / np.linalg.norm(ref_cov[s, s])))
    return out


def check_ok(got, status, ref, bars=BARS, where=""):
    """An implementation's matrix of a window whose reference is regular: status OK, symmetric to the last bit, positive diagonals on
    the free keyframes, zero rows and columns elsewhere, both classes inside their bars (None: measure only).  Returns the deviations."""
    assert status == OK, (where, status)
    assert not ref.rank_deficient, where
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes(), (where, "not symmetric to the last bit")
    n_kf = got.shape[0] // 6
    for k in range(n_kf):
        s = slice(6 * k, 6 * k + 6)
        if k in ref.free:
            assert (np.diag(got)[s] > 0).all(), (where, k)
        else:
            assert not got[s, :].any() and not got[:, s].any(), (where, k)
    dev = deviation(got, ref.cov, ref.free)
    if bars is not None:
        for cls, v in dev.items():
            assert v <= bars[cls], (where, cls, "%.3e > %.1e" % (v, bars[cls]))
    return dev


# ------------------------------------------------------------------------------------------------ the cases
def no_trim_options(**over):
    return default_options(num_trim_rounds=0, **over)


TRIMMED_SEEDS = (7400, 7300)  # default options: 10 and 22 landmarks trimmed
RANK_DEFICIENT_SEED = 7306    # a free keyframe without a view
POSE_WINDOWS = ("71", "71_none", "71_small")
FIXED_WINDOWS = ("a", "b", "e_all", "h_b_02")
NOTHING_VARIABLE = "f"
EACH_SCALES = ((0.16, 1.6), (0.5, 5.0))  # (depth_thres, reprojection_thres) of the two windows of the solve_each batch
EACH_SEEDS = (7102, 7401)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (w0 factory, options, problem factory or None).  The factories return fresh copies."""
    out = {}
    for c in lsc.SHAPES:
        seed = c["seed"]
        out["shape_%d" % seed] = (functools.partial(lsc.window, seed), no_trim_options(), None)
    for seed in TRIMMED_SEEDS:
        out["trimmed_%d" % seed] = (functools.partial(lsc.window, seed), default_options(), None)
    for name in POSE_WINDOWS:
        out["pose_" + name] = (functools.partial(_pose_w, name), no_trim_options(), functools.partial(_pose_p, name))
    for name in FIXED_WINDOWS + (NOTHING_VARIABLE,):
        out["fixed_" + name] = (functools.partial(_fixed_w, name), no_trim_options(), functools.partial(_fixed_p, name))
    for seed in lsc.SMALL:
        out["unscaled_%d" % seed] = (functools.partial(lsc.window, seed), no_trim_options(jacobi_scaling=0), None)
    for seed, (dt, rt) in zip(EACH_SEEDS, EACH_SCALES):
        out["each_%d" % seed] = (functools.partial(lsc.window, seed), no_trim_options(depth_thres=dt, reprojection_thres=rt), None)
    return out


def _pose_w(name):
    return lsc.pose_window(name)[0]


def _pose_p(name):
    return lsc.pose_window(name)[1]


def _fixed_w(name):
    return lsc.fixed_window(name)[0]


def _fixed_p(name):
    return lsc.fixed_window(name)[1]


def case(name):
    """(w0, options, problem) of a case."""
    w, o, p = cases()[name]
    return w(), o, (lsc.SOLVE if p is None else p())


def expected_status(name):
    if name == "shape_%d" % RANK_DEFICIENT_SEED:
        return RANK_DEFICIENT
    if name == "fixed_" + NOTHING_VARIABLE:
        return NO_FREE_POSE
    return OK


_emu_cache = {}


def emu_case(name):
    """The emulator on a case, computed once: (w0, final, report, matrix, status, trimmed)."""
    if name not in _emu_cache:
        w0, o, problem = case(name)
        final = w0.copy()
        reps, mats, status, trimmed = emu_solve([final], o, problem)
        for a in (mats[0], trimmed[0]):
            a.setflags(write=False)
        _emu_cache[name] = (w0, final, reps[0], mats[0], status[0], trimmed[0])
    return _emu_cache[name]


_ref_cache = {}


def reference(name, final, trimmed):
    """The reference of a case at an implementation's final window (cached per final point)."""
    key = (name, final.kf_pose.tobytes(), final.lm_pos.tobytes(), final.kf_plane_dir.tobytes(), final.kf_plane_dist.tobytes(), tuple(int(t) for t in trimmed))
    if key not in _ref_cache:
        w0, o, problem = case(name)
        _ref_cache[key] = Reference(w0, final, o, problem, trimmed)
    return _ref_cache[key]
