"""Thin Python driver over the C-ABI (ctypes): context, batched solve, evaluate, pose-only.

Used by tests and bench.py.  It never computes anything itself: every call goes through
`limo_amd/lib/liblimo_hip.so` (include/limo_hip.h) and fails loudly if that library or a GPU is missing.
"""
import ctypes as C

import numpy as np

from . import _ffi
from .window import struct_array


class LimoError(RuntimeError):
    pass


class NotEnoughKeyframes(LimoError):
    """BundleAdjusterKeyframes::NotEnoughKeyframesException (bundle_adjuster_keyframes.hpp:59-68)."""


def _check(rc, ctx=None, what=""):
    if rc == _ffi.LIMO_OK:
        return
    msg = ""
    if ctx is not None:
        msg = _ffi.load().limo_last_error(ctx).decode(errors="replace")
    if rc == _ffi.LIMO_ERR_NOT_ENOUGH_KF:
        raise NotEnoughKeyframes(msg or what)
    raise LimoError("%s failed: rc=%d %s" % (what, rc, msg))


class Context:
    def __init__(self, device=0, stream=None):
        self.lib = _ffi.load()
        self.device = device
        self._last_n_kf = []  # keyframes of the windows of the last call that owned its batch (last_pose_covariance)
        self.ptr = C.c_void_p()
        rc = self.lib.limo_ctx_create(device, C.byref(self.ptr))
        if rc != 0:
            raise LimoError("limo_ctx_create(device=%d) failed rc=%d (no gfx950 device? the product path has no CPU fallback)" % (device, rc))
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        _check(self.lib.limo_ctx_set_stream(self.ptr, C.c_void_p(stream)), self.ptr, "limo_ctx_set_stream")

    def close(self):
        if self.ptr:
            self.lib.limo_ctx_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- single window
    def solve(self, window, opts, lm_fixed=None):
        """limo_ba_solve; lm_fixed (one flag per landmark, non-zero = constant parameter block): limo_ba_solve_fixed_landmarks."""
        s = window.as_struct()
        rep = _ffi.BaReport()
        self._last_n_kf = [window.n_kf]
        if lm_fixed is not None:
            flags = fixed_flags(lm_fixed, window.n_lm)
            rc = self.lib.limo_ba_solve_fixed_landmarks(self.ptr, C.byref(s), flags.ctypes.data_as(_ffi.c_uint8_p), C.byref(opts), C.byref(rep))
            _check(rc, self.ptr, "limo_ba_solve_fixed_landmarks")
            return rep.as_dict()
        _check(self.lib.limo_ba_solve(self.ptr, C.byref(s), C.byref(opts), C.byref(rep)), self.ptr, "limo_ba_solve")
        return rep.as_dict()

    def solve_sharded(self, window, opts, n_shards):
        """Landmark-sharded solve of one window: ranks of the communicator set by comm_init(), or
        n_shards virtual shards on this GPU when there is none."""
        s = window.as_struct()
        rep = _ffi.BaReport()
        self._last_n_kf = [window.n_kf]
        _check(self.lib.limo_ba_solve_sharded(self.ptr, C.byref(s), C.byref(opts), int(n_shards), C.byref(rep)), self.ptr, "limo_ba_solve_sharded")
        return rep.as_dict()

    def exchange_stats(self):
        """limo_ctx_exchange_stats of the last solve_sharded: dict(exchanges, bytes, iterations)."""
        st = (C.c_int64 * 3)()
        _check(self.lib.limo_ctx_exchange_stats(self.ptr, st), self.ptr, "limo_ctx_exchange_stats")
        return {"exchanges": int(st[0]), "bytes": int(st[1]), "iterations": int(st[2])}

    def coop_fallbacks(self):
        """limo_ctx_coop_fallbacks: one-launch solves on this context that timed out at a barrier and were redone as launches."""
        return int(self.lib.limo_ctx_coop_fallbacks(self.ptr))

    SOLVE_PATHS = {1: "WG", 2: "COOP", 3: "STREAMING", 4: "LOCKSTEP"}

    def last_solve_info(self):
        """limo_ctx_last_solve_info: which launch path the last solve on this context took (path: WG, COOP, STREAMING or LOCKSTEP)
        and what it launched."""
        v = (C.c_int64 * 8)()
        _check(self.lib.limo_ctx_last_solve_info(self.ptr, v), self.ptr, "limo_ctx_last_solve_info")
        keys = ("recovered", "coop_G", "groups", "slots", "rounds", "pair_launches", "lin_variant")
        return dict({"path": self.SOLVE_PATHS.get(int(v[0]), "NONE")}, **{k: int(v[1 + i]) for i, k in enumerate(keys)})

    def last_schur_gp_info(self):
        """limo_ctx_last_schur_gp_info: narrow / wide ground-plane Schur groups of the batch of the last solve on this context and the
        launches that ran narrow / three-panel ground-plane waves."""
        v = (C.c_int64 * 4)()
        _check(self.lib.limo_ctx_last_schur_gp_info(self.ptr, v), self.ptr, "limo_ctx_last_schur_gp_info")
        return dict(zip(("narrow_groups", "wide_groups", "narrow_launches", "wide_launches"), (int(x) for x in v)))

    def last_cam_lanes_info(self):
        """limo_ctx_last_cam_lanes_info: how many launches of k_cam_assemble / k_cam_solve of the last solve on this context ran with
        128 and with 256 lanes per window, the workgroups per compute unit of the four instances, and the windows of the batch whose
        camera system works in global memory."""
        v = (C.c_int64 * 9)()
        _check(self.lib.limo_ctx_last_cam_lanes_info(self.ptr, v), self.ptr, "limo_ctx_last_cam_lanes_info")
        keys = ("assemble_128", "assemble_256", "solve_128", "solve_256", "wg_per_cu_assemble_128", "wg_per_cu_assemble_256",
                "wg_per_cu_solve_128", "wg_per_cu_solve_256", "global_class_windows")
        return dict(zip(keys, (int(x) for x in v)))

    def set_iteration_log(self, on):
        """limo_ctx_set_iteration_log: the solves on this context record Ceres' per-iteration table (off by default)."""
        _check(self.lib.limo_ctx_set_iteration_log(self.ptr, int(bool(on))), self.ptr, "limo_ctx_set_iteration_log")

    def last_iteration_log(self, window=0):
        """limo_ctx_last_iteration_log: the entries of window `window` of the last solve / adjust_pose_only[_batch] call on this
        context, as a numpy array of _ffi.iteration_dtype() (empty with the switch off)."""
        return _read_iteration_log(lambda cap, out, n: self.lib.limo_ctx_last_iteration_log(self.ptr, int(window), cap, out, n), self.ptr,
                                   "limo_ctx_last_iteration_log")

    def set_pose_covariance(self, on):
        """limo_ctx_set_pose_covariance: every solve on this context ends with the marginal pose covariance of its windows (off by
        default; changes no result of a solve)."""
        _check(self.lib.limo_ctx_set_pose_covariance(self.ptr, int(bool(on))), self.ptr, "limo_ctx_set_pose_covariance")

    def last_pose_covariance(self, window=0):
        """limo_ctx_last_pose_covariance: (matrix [6 n_kf, 6 n_kf] or None, status) of window `window` of the last solve /
        adjust_pose_only[_batch] call on this context (the context remembers the keyframe counts of that call's windows).  The matrix
        is None for LIMO_COV_NOT_COMPUTED.  Tangent units: include/limo_hip.h, "Pose covariance"."""
        n_kf = self._last_n_kf[window] if 0 <= window < len(self._last_n_kf) else 1
        return _read_pose_covariance(lambda cap, out, st: self.lib.limo_ctx_last_pose_covariance(self.ptr, int(window), cap, out, st), n_kf, self.ptr,
                                     "limo_ctx_last_pose_covariance")

    def comm_init(self, unique_id, rank, world):
        _check(self.lib.limo_ctx_comm_init(self.ptr, unique_id, int(rank), int(world)), self.ptr, "limo_ctx_comm_init")

    def comm_init_host(self, rank, world, allgather, allreduce):
        """limo_ctx_comm_init_host: the exchange steps of solve_sharded through the caller's transport, staged in host memory.
        allgather(send[count], recv[world, count]) / allreduce(send[count], recv[count]) get numpy views of the staging buffers."""
        import numpy as np

        def _cb(send, recv, count, kind, _user):
            s = np.ctypeslib.as_array(send, shape=(count,))
            if kind == 0:
                allgather(s, np.ctypeslib.as_array(recv, shape=(world, count)))
            else:
                allreduce(s, np.ctypeslib.as_array(recv, shape=(count,)))

        self._xfn = _ffi.EXCHANGE_FN(_cb)  # (kept alive with the context)
        _check(self.lib.limo_ctx_comm_init_host(self.ptr, self._xfn, None, int(rank), int(world)), self.ptr, "limo_ctx_comm_init_host")

    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        _check(self.lib.limo_comm_unique_id(buf), self.ptr, "limo_comm_unique_id")
        return buf.raw

    def landmark_init(self, ray_off, rays, use_depth):
        """limo_landmark_init: rays = ctypes array of _ffi.Ray (CSR by ray_off); returns (positions [n,3], ok [n])."""
        ray_off = np.ascontiguousarray(ray_off, np.int32)
        use_depth = np.ascontiguousarray(use_depth, np.uint8)
        n = len(use_depth)
        pos = np.zeros((n, 3))
        ok = np.zeros(n, np.uint8)
        rc = self.lib.limo_landmark_init(self.ptr, n, ray_off.ctypes.data_as(_ffi.c_int32_p), rays, use_depth.ctypes.data_as(_ffi.c_uint8_p),
                                         pos.ctypes.data_as(_ffi.c_double_p), ok.ctypes.data_as(_ffi.c_uint8_p))
        _check(rc, self.ptr, "limo_landmark_init")
        return pos, ok

    def five_point_params(self, probability=None, threshold_px=None, max_samples=None, chunk=None):
        """limo_five_point_default_params, with the given fields replaced."""
        p = _ffi.FivePointParams()
        self.lib.limo_five_point_default_params(C.byref(p))
        for name, v in (("probability", probability), ("threshold_px", threshold_px), ("max_samples", max_samples), ("chunk", chunk)):
            if v is not None:
                setattr(p, name, v)
        return p

    def five_point(self, pts_a, pts_b, focal, cx, cy, seed=1, params=None, with_mask=False):
        """limo_five_point: relative motion x_b = R x_a + t from matches pts_a / pts_b ([n, 2] pixels).  Returns the Motion as a
        dict (plus "raw": the struct's bytes, "inlier": the mask with with_mask)."""
        a = np.ascontiguousarray(pts_a, np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(pts_b, np.float64).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("five_point: %d points in a, %d in b" % (len(a), len(b)))
        fr = _ffi.FivePointFrame(len(a), a.ctypes.data_as(_ffi.c_double_p), b.ctypes.data_as(_ffi.c_double_p), int(seed))
        p = params if params is not None else self.five_point_params()
        m = _ffi.FivePointMotion()
        mask = np.zeros(max(1, len(a)), np.uint8) if with_mask else None
        rc = self.lib.limo_five_point(self.ptr, C.byref(fr), float(focal), float(cx), float(cy), C.byref(p), C.byref(m),
                                      mask.ctypes.data_as(_ffi.c_uint8_p) if with_mask else None)
        _check(rc, self.ptr, "limo_five_point")
        out = m.as_dict()
        out["raw"] = bytes(m)
        if with_mask:
            out["inlier"] = mask[: len(a)]
        return out

    def five_point_batch(self, frames, focal, cx, cy, params=None):
        """limo_five_point_batch: frames = [(pts_a, pts_b, seed), ...]; one dict per frame, as five_point returns it."""
        keep = [(np.ascontiguousarray(a, np.float64).reshape(-1, 2), np.ascontiguousarray(b, np.float64).reshape(-1, 2), int(s)) for a, b, s in frames]
        n = len(keep)
        arr = (_ffi.FivePointFrame * max(1, n))()
        for i, (a, b, s) in enumerate(keep):
            if len(a) != len(b):
                raise ValueError("five_point_batch: frame %d: %d points in a, %d in b" % (i, len(a), len(b)))
            arr[i] = _ffi.FivePointFrame(len(a), a.ctypes.data_as(_ffi.c_double_p), b.ctypes.data_as(_ffi.c_double_p), s)
        p = params if params is not None else self.five_point_params()
        ms = (_ffi.FivePointMotion * max(1, n))()
        _check(self.lib.limo_five_point_batch(self.ptr, n, arr, float(focal), float(cx), float(cy), C.byref(p), ms), self.ptr, "limo_five_point_batch")
        out = []
        for i in range(n):
            d = ms[i].as_dict()
            d["raw"] = bytes(ms[i])
            out.append(d)
        return out

    def select_params(self, add=(), **fields):
        """limo_select_default_params with the given fields replaced (voxel_size_xyz, roi_far, roi_middle, max_near, max_middle, max_far,
        sort_capacity); add = [(frame_index, count, predicate, key), ...] is the must-have list."""
        p = _ffi.SelectParams()
        self.lib.limo_select_default_params(C.byref(p))
        for name, v in fields.items():
            if name == "voxel_size_xyz":
                p.voxel_size_xyz[:] = [float(x) for x in v]
            else:
                setattr(p, name, v)
        if len(add):
            p._add_keep = (_ffi.SelectAdd * len(add))(*[_ffi.SelectAdd(*(int(x) for x in a)) for a in add])  # (kept alive with the struct)
            p.add, p.n_add = p._add_keep, len(add)
        return p

    def landmark_select(self, pool, params=None):
        """limo_landmark_select: pool = dict of arrays (see _ffi.select_pool).  Returns one byte per landmark: low two bits 0 not chosen
        by the voxel scheme / 1 near / 2 middle / 3 far, | 4 must-have, 8 rejected by cheirality; selected iff byte & 7."""
        w, keep = _ffi.select_pool(pool)
        p = params if params is not None else self.select_params()
        out = np.zeros(max(1, w.n_lm), np.uint8)
        _check(self.lib.limo_landmark_select(self.ptr, C.byref(w), C.byref(p), out.ctypes.data_as(_ffi.c_uint8_p)), self.ptr, "limo_landmark_select")
        del keep
        return out[: w.n_lm]

    def landmark_select_batch(self, pools, params=None):
        """limo_landmark_select_batch: one byte array per pool, the bytes of its single call."""
        n = len(pools)
        arr = (_ffi.SelectPool * max(1, n))()
        keep, outs = [], []
        for i, pool in enumerate(pools):
            arr[i], k = _ffi.select_pool(pool)
            keep.append(k)
            outs.append(np.zeros(max(1, arr[i].n_lm), np.uint8))
        ptrs = (_ffi.c_uint8_p * max(1, n))(*[o.ctypes.data_as(_ffi.c_uint8_p) for o in outs])
        p = params if params is not None else self.select_params()
        _check(self.lib.limo_landmark_select_batch(self.ptr, n, arr, C.byref(p), ptrs), self.ptr, "limo_landmark_select_batch")
        del keep
        return [o[: arr[i].n_lm] for i, o in enumerate(outs)]

    def select_kernel_ms(self):
        """limo_select_last_kernel_ms: device time of the kernels of the last landmark_select[_batch] call (after set_select_timing(True))."""
        ms = C.c_double(0.0)
        _check(self.lib.limo_select_last_kernel_ms(self.ptr, C.byref(ms)), self.ptr, "limo_select_last_kernel_ms")
        return ms.value

    def set_select_timing(self, on):
        _check(self.lib.limo_select_set_timing(self.ptr, int(bool(on))), self.ptr, "limo_select_set_timing")

    def adjust_pose_only(self, window, prior, opts):
        s = window.as_struct()
        rep = _ffi.BaReport()
        self._last_n_kf = [window.n_kf]
        rc = self.lib.limo_ba_adjust_pose_only(self.ptr, C.byref(s), None if prior is None else C.byref(prior), C.byref(opts), C.byref(rep))
        _check(rc, self.ptr, "limo_ba_adjust_pose_only")
        return rep.as_dict()

    def adjust_pose_only_batch(self, windows, priors, opts):
        """limo_ba_adjust_pose_only_batch: N independent pose-only windows in one call.  priors: None, or one entry per window
        (a _ffi.SpeedPrior, or None for a window without prior).  opts: one BaOptions, or a sequence with one per window (thresholds and
        quantiles may differ, include/limo_hip.h).  The windows' poses are updated in place; returns the reports."""
        windows = list(windows)
        arr = struct_array(windows)
        reps = (_ffi.BaReport * max(1, len(windows)))()
        self._last_n_kf = [w.n_kf for w in windows]
        if not isinstance(opts, _ffi.BaOptions):  # a sequence: one set of options per window (limo_ba_adjust_pose_only_batch_each)
            each, n_each = options_array(opts)
            if n_each != len(windows):
                raise ValueError("opts: %d entries for %d windows" % (n_each, len(windows)))
            rc = self.lib.limo_ba_adjust_pose_only_batch_each(self.ptr, len(windows), arr, prior_array(priors, len(windows)), each, reps)
            _check(rc, self.ptr, "limo_ba_adjust_pose_only_batch_each")
            return [reps[i].as_dict() for i in range(len(windows))]
        rc = self.lib.limo_ba_adjust_pose_only_batch(self.ptr, len(windows), arr, prior_array(priors, len(windows)), C.byref(opts), reps)
        _check(rc, self.ptr, "limo_ba_adjust_pose_only_batch")
        return [reps[i].as_dict() for i in range(len(windows))]

    def evaluate(self, window, opts, apply_loss=True):
        s = window.as_struct()
        M = window.n_obs
        cost = np.zeros(1)
        res = np.zeros((M, 3))
        jp = np.zeros((M, 3, 6))
        jl = np.zeros((M, 3, 3))
        valid = np.zeros(M, np.uint8)
        dp = lambda a: a.ctypes.data_as(_ffi.c_double_p)
        rc = self.lib.limo_ba_evaluate(self.ptr, C.byref(s), C.byref(opts), int(apply_loss), dp(cost), dp(res), dp(jp), dp(jl), valid.ctypes.data_as(_ffi.c_uint8_p))
        _check(rc, self.ptr, "limo_ba_evaluate")
        return float(cost[0]), res, jp, jl, valid


    def evaluate_rows(self, window, opts, pose_only=False, prior=None):
        """limo_ba_evaluate_rows: the non-observation residual rows (ground plane, regularisers, speed prior) as dicts."""
        s = window.as_struct()
        n = C.c_int32(0)
        cap = 64 + window.n_lm + 8 * window.n_kf
        rows = (_ffi.BaRow * cap)()
        rc = self.lib.limo_ba_evaluate_rows(self.ptr, C.byref(s), None if prior is None else C.byref(prior), int(pose_only), C.byref(opts), cap, rows, C.byref(n))
        _check(rc, self.ptr, "limo_ba_evaluate_rows")
        assert n.value <= cap
        return _ffi.rows_as_dicts(rows, n.value)


def _read_iteration_log(call, ctx_ptr, what):
    """Both readers of the iteration log: ask for the count, then for the entries."""
    n = C.c_int32(0)
    _check(call(0, None, C.byref(n)), ctx_ptr, what)
    out = np.zeros(n.value, _ffi.iteration_dtype())
    if n.value:
        _check(call(n.value, out.ctypes.data_as(C.POINTER(_ffi.BaIteration)), C.byref(n)), ctx_ptr, what)
        assert n.value == out.size
    return out


def _read_pose_covariance(call, n_kf, ctx_ptr, what):
    """Both readers of the pose covariance: the status first, then the matrix."""
    st = C.c_int32(_ffi.LIMO_COV_NOT_COMPUTED)
    _check(call(0, None, C.byref(st)), ctx_ptr, what)
    if st.value == _ffi.LIMO_COV_NOT_COMPUTED:
        return None, st.value
    out = np.zeros((6 * n_kf, 6 * n_kf))
    _check(call(out.size, out.ctypes.data_as(_ffi.c_double_p), C.byref(st)), ctx_ptr, what)
    return out, st.value


def fixed_flags(lm_fixed, n_lm):
    """One uint8 flag per landmark of a window (non-zero: constant), contiguous, at least one byte long."""
    flags = np.ascontiguousarray(lm_fixed).astype(bool).astype(np.uint8).ravel()
    if flags.size != n_lm:
        raise ValueError("lm_fixed: %d flags for %d landmarks" % (flags.size, n_lm))
    return flags if n_lm else np.zeros(1, np.uint8)


def options_array(opts):
    """(limo_ba_options[n], n) from a sequence of _ffi.BaOptions (copies; the array is at least one entry long)."""
    opts = list(opts)
    arr = (_ffi.BaOptions * max(1, len(opts)))()
    for i, o in enumerate(opts):
        C.memmove(C.byref(arr, i * C.sizeof(_ffi.BaOptions)), C.byref(o), C.sizeof(_ffi.BaOptions))
    return arr, len(opts)


def prior_array(priors, n):
    """limo_speed_prior[n] for a list of _ffi.SpeedPrior / None (None: speed_weight 0, no prior for that window); None for priors=None."""
    if priors is None:
        return None
    priors = list(priors)
    if len(priors) != n:
        raise ValueError("priors: %d entries for %d windows" % (len(priors), n))
    arr = (_ffi.SpeedPrior * max(1, n))()
    for i, p in enumerate(priors):
        if p is not None:
            arr[i] = p
    return arr


class Batch:
    """Many independent windows resident in HBM (limo_ba_batch_*)."""

    def __init__(self, ctx, windows, arr=None, pose_only=False, priors=None, lm_fixed=None):
        """arr: struct_array(windows) made earlier (the array of limo_ba_window a C / C++ caller holds anyway: building it from
        numpy windows is ~20 us of Python per window and not part of the library call).
        pose_only=True: every window is an adjustPoseOnly problem (limo_ba_batch_create_pose_only), priors = None or one
        _ffi.SpeedPrior / None per window.
        lm_fixed: None, or one entry per window, each None or that window's per-landmark flags (non-zero: the landmark is a constant
        parameter block) - limo_ba_batch_create_fixed_landmarks."""
        self.ctx = ctx
        self.lib = ctx.lib
        self.windows = list(windows)
        self._arr = struct_array(self.windows) if arr is None else arr
        self.ptr = C.c_void_p()
        if pose_only:
            if lm_fixed is not None:
                raise ValueError("lm_fixed belongs to a solve batch: the landmarks of a pose_only batch are all constant")
            rc = self.lib.limo_ba_batch_create_pose_only(ctx.ptr, len(self.windows), self._arr, prior_array(priors, len(self.windows)), C.byref(self.ptr))
            _check(rc, ctx.ptr, "limo_ba_batch_create_pose_only")
            return
        if priors is not None:
            raise ValueError("priors belong to a pose_only batch")
        if lm_fixed is not None:
            lm_fixed = list(lm_fixed)
            if len(lm_fixed) != len(self.windows):
                raise ValueError("lm_fixed: %d entries for %d windows" % (len(lm_fixed), len(self.windows)))
            keep = [None if f is None else fixed_flags(f, w.n_lm) for f, w in zip(lm_fixed, self.windows)]
            ptrs = (_ffi.c_uint8_p * max(1, len(keep)))(*[None if f is None else f.ctypes.data_as(_ffi.c_uint8_p) for f in keep])
            rc = self.lib.limo_ba_batch_create_fixed_landmarks(ctx.ptr, len(self.windows), self._arr, ptrs, C.byref(self.ptr))
            _check(rc, ctx.ptr, "limo_ba_batch_create_fixed_landmarks")
            return
        _check(self.lib.limo_ba_batch_create(ctx.ptr, len(self.windows), self._arr, C.byref(self.ptr)), ctx.ptr, "limo_ba_batch_create")

    def solve(self, opts):
        """opts: one BaOptions for all windows, or a sequence with one per window (limo_ba_batch_solve_each: thresholds and quantiles may
        differ from window to window, everything else must be equal)."""
        if isinstance(opts, _ffi.BaOptions):
            _check(self.lib.limo_ba_batch_solve(self.ptr, C.byref(opts)), self.ctx.ptr, "limo_ba_batch_solve")
            return
        each, n_each = options_array(opts)
        _check(self.lib.limo_ba_batch_solve_each(self.ptr, n_each, each), self.ctx.ptr, "limo_ba_batch_solve_each")

    def reset(self):
        _check(self.lib.limo_ba_batch_reset(self.ptr), self.ctx.ptr, "limo_ba_batch_reset")

    def download(self):
        """Writes optimised parameters into self.windows (in place) and returns the reports."""
        reps = (_ffi.BaReport * len(self.windows))()
        _check(self.lib.limo_ba_batch_download(self.ptr, self._arr, reps), self.ctx.ptr, "limo_ba_batch_download")
        return [r.as_dict() for r in reps]

    def trimmed(self, w=0):
        """Indices (caller's order) of the landmarks of window w removed by the trimming rounds of the last solve."""
        flags = np.zeros(max(1, self.windows[w].n_lm), np.uint8)
        _check(self.lib.limo_ba_batch_trimmed(self.ptr, int(w), flags.ctypes.data_as(_ffi.c_uint8_p)), self.ctx.ptr, "limo_ba_batch_trimmed")
        return np.nonzero(flags[: self.windows[w].n_lm])[0].astype(np.int32)

    def iteration_log(self, w=0):
        """limo_ba_batch_iteration_log: the entries window w recorded in the last solve of this batch, as a numpy array of
        _ffi.iteration_dtype() (empty when the context's switch was off)."""
        return _read_iteration_log(lambda cap, out, n: self.lib.limo_ba_batch_iteration_log(self.ptr, int(w), cap, out, n), self.ctx.ptr,
                                   "limo_ba_batch_iteration_log")

    def pose_covariance(self, w=0):
        """limo_ba_batch_pose_covariance: (matrix [6 n_kf, 6 n_kf] or None, status) of window w after the last solve of this batch
        (None, LIMO_COV_NOT_COMPUTED when the context's switch was off)."""
        return _read_pose_covariance(lambda cap, out, st: self.lib.limo_ba_batch_pose_covariance(self.ptr, int(w), cap, out, st), self.windows[w].n_kf,
                                     self.ctx.ptr, "limo_ba_batch_pose_covariance")

    def kernel_stats(self, reset=False):
        ms = C.c_double()
        n = C.c_int64()
        tot = C.c_double()
        sms, sn = C.c_double(), C.c_int64()
        _check(self.lib.limo_ba_batch_kernel_time(self.ptr, 1, C.byref(sms), C.byref(sn)), self.ctx.ptr, "limo_ba_batch_kernel_time")
        out = {"schur_ms": sms.value, "schur_launches": sn.value}
        _check(self.lib.limo_ba_batch_kernel_stats(self.ptr, int(reset), C.byref(ms), C.byref(n), C.byref(tot)), self.ctx.ptr, "limo_ba_batch_kernel_stats")
        out.update({"linearize_ms": ms.value, "linearize_launches": n.value, "total_ms": tot.value})
        return out

    def close(self):
        if self.ptr:
            self.lib.limo_ba_batch_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def evaluate_batch_time(ctx, windows, opts, reps=10):
    """limo_ba_evaluate_batch_time: device ms of one k_evaluate launch over `windows`; returns (ms, n_obs, n_depth_obs)."""
    arr = struct_array(windows)
    ms = C.c_double()
    _check(ctx.lib.limo_ba_evaluate_batch_time(ctx.ptr, len(windows), arr, C.byref(opts), int(reps), C.byref(ms)), ctx.ptr, "limo_ba_evaluate_batch_time")
    return ms.value, int(sum(w.n_obs for w in windows)), int(sum((w.obs_d > 0).sum() for w in windows))


def depth_default_params():
    p = _ffi.DepthParams()
    _ffi.load().limo_depth_default_params(C.byref(p))
    return p


def depth_estimate(ctx, frame, params=None, use_ground_labels=True):
    """limo_depth_estimate on one frame dict (see limo_amd.synth_lidar.make_frame): returns float32 depth per feature."""
    lib = ctx.lib
    p = params if params is not None else depth_default_params()
    cloud = np.ascontiguousarray(frame["cloud"], np.float32)
    uv = np.ascontiguousarray(frame["uv"], np.float32)
    T = np.ascontiguousarray(frame["T_cam_lidar"], np.float64)
    g = np.ascontiguousarray(frame["is_ground"], np.uint8) if use_ground_labels else None
    out = np.zeros(uv.shape[0], np.float32)
    rc = lib.limo_depth_estimate(
        ctx.ptr,
        cloud.ctypes.data_as(_ffi.c_float_p),
        cloud.shape[0],
        T.ctypes.data_as(_ffi.c_double_p),
        frame["f"],
        frame["cx"],
        frame["cy"],
        frame["w"],
        frame["h"],
        uv.ctypes.data_as(_ffi.c_float_p),
        uv.shape[0],
        None if g is None else g.ctypes.data_as(_ffi.c_uint8_p),
        C.byref(p),
        out.ctypes.data_as(_ffi.c_float_p),
    )
    _check(rc, ctx.ptr, "limo_depth_estimate")
    return out


def depth_estimate_begin(ctx, frame, params=None, use_ground_labels=True):
    """limo_depth_estimate_begin: the frame's depth assignment is enqueued on the context's stream; returns the handle
    depth_estimate_end wants (it keeps the cloud alive until then)."""
    p = params if params is not None else depth_default_params()
    cloud = np.ascontiguousarray(frame["cloud"], np.float32)
    uv = np.ascontiguousarray(frame["uv"], np.float32)
    T = np.ascontiguousarray(frame["T_cam_lidar"], np.float64)
    g = np.ascontiguousarray(frame["is_ground"], np.uint8) if use_ground_labels else None
    rc = ctx.lib.limo_depth_estimate_begin(
        ctx.ptr, cloud.ctypes.data_as(_ffi.c_float_p), cloud.shape[0], T.ctypes.data_as(_ffi.c_double_p), frame["f"], frame["cx"], frame["cy"],
        frame["w"], frame["h"], uv.ctypes.data_as(_ffi.c_float_p), uv.shape[0], None if g is None else g.ctypes.data_as(_ffi.c_uint8_p), C.byref(p))
    _check(rc, ctx.ptr, "limo_depth_estimate_begin")
    return (cloud, uv.shape[0])


def depth_estimate_end(ctx, handle):
    """limo_depth_estimate_end: float32 depth per feature of the frame given to depth_estimate_begin."""
    out = np.zeros(handle[1], np.float32)
    _check(ctx.lib.limo_depth_estimate_end(ctx.ptr, out.ctypes.data_as(_ffi.c_float_p), handle[1]), ctx.ptr, "limo_depth_estimate_end")
    return out


def depth_kernel_ms(ctx):
    """limo_depth_last_kernel_ms (after limo_depth_set_timing(ctx, 1)): dict of device milliseconds of the last launch group."""
    ms = np.zeros(4)
    _check(ctx.lib.limo_depth_last_kernel_ms(ctx.ptr, ms.ctypes.data_as(_ffi.c_double_p)), ctx.ptr, "limo_depth_last_kernel_ms")
    return {"k_project": ms[0], "ground_plane": ms[1], "k_features": ms[2], "total": ms[3]}


def depth_last_ground_plane(ctx, frame=0):
    """limo_depth_last_ground_plane: (RANSAC inliers, plane4) of a frame of the last depth call on this context."""
    pl = np.zeros(4)
    n = C.c_int32(0)
    rc = ctx.lib.limo_depth_last_ground_plane(ctx.ptr, frame, pl.ctypes.data_as(_ffi.c_double_p), C.byref(n))
    _check(rc, ctx.ptr, "limo_depth_last_ground_plane")
    return n.value, pl


def depth_last_reasons(ctx, n_feat, frame=0):
    """limo_depth_last_reasons: the gate that decided each of the n_feat features of a frame of the last depth call on
    this context (uint8 array of _ffi.DEPTH_* codes)."""
    out = np.zeros(n_feat, np.uint8)
    rc = ctx.lib.limo_depth_last_reasons(ctx.ptr, frame, out.ctypes.data_as(_ffi.c_uint8_p), n_feat)
    _check(rc, ctx.ptr, "limo_depth_last_reasons")
    return out


def depth_estimate_batch(ctx, frames, params=None, use_ground_labels=True, device=False):
    """limo_depth_estimate_batch over a list of frame dicts of one rig (calibration of frames[0]).
    device=False: numpy clouds / features in, list of float32 depth arrays out.
    device=True: every frame dict carries torch CUDA tensors "cloud" (n,4 float32), "uv" (m,2 float32), optionally
    "is_ground" (m uint8); returns a list of torch CUDA float32 tensors (nothing crosses PCIe)."""
    lib = ctx.lib
    p = params if params is not None else depth_default_params()
    n = len(frames)
    arr = (_ffi.DepthFrame * max(1, n))()
    keep, outs = [], []
    for k, fr in enumerate(frames):
        if device:
            import torch

            cloud, uv = fr["cloud"].contiguous(), fr["uv"].contiguous()
            assert cloud.is_cuda and cloud.dtype == torch.float32 and uv.is_cuda and uv.dtype == torch.float32
            g = fr["is_ground"].contiguous() if use_ground_labels and fr.get("is_ground") is not None else None
            out = torch.empty(uv.shape[0], dtype=torch.float32, device=uv.device)
            arr[k] = _ffi.DepthFrame(cloud.data_ptr(), cloud.shape[0], uv.data_ptr(), uv.shape[0], g.data_ptr() if g is not None else None, out.data_ptr())
        else:
            cloud = np.ascontiguousarray(fr["cloud"], np.float32)
            uv = np.ascontiguousarray(fr["uv"], np.float32)
            g = np.ascontiguousarray(fr["is_ground"], np.uint8) if use_ground_labels else None
            out = np.zeros(uv.shape[0], np.float32)
            arr[k] = _ffi.DepthFrame(cloud.ctypes.data, cloud.shape[0], uv.ctypes.data, uv.shape[0], g.ctypes.data if g is not None else None, out.ctypes.data)
        keep.append((cloud, uv, g))
        outs.append(out)
    if n == 0:
        return []
    f0 = frames[0]
    T = np.ascontiguousarray(f0["T_cam_lidar"], np.float64)
    if device:
        import torch

        torch.cuda.current_stream().synchronize()  # the tensors above may still be in flight on torch's stream
    rc = lib.limo_depth_estimate_batch(ctx.ptr, n, arr, T.ctypes.data_as(_ffi.c_double_p), f0["f"], f0["cx"], f0["cy"], f0["w"], f0["h"], C.byref(p),
                                       _ffi.DEPTH_DEVICE_POINTERS if device else 0)
    _check(rc, ctx.ptr, "limo_depth_estimate_batch")
    return outs


def host_array(shape, dtype):
    """numpy array on page-locked host memory (limo_host_alloc); freed when the array is collected."""
    lib = _ffi.load()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    ptr = lib.limo_host_alloc(max(1, n))
    if not ptr:
        raise MemoryError("limo_host_alloc(%d)" % n)

    class _Owner:
        def __del__(self, free=lib.limo_host_free, p=ptr):
            free(p)

    buf = (C.c_char * max(1, n)).from_address(ptr)
    buf._owner = _Owner()
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
