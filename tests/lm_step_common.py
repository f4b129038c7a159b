"""One Levenberg-Marquardt step of the windowed solve held to a dense reference, shared by the CPU tier (tests/test_lm_step_cpu.py:
the emulator and the oracle's own Schur-based solve) and the GPU tier (tests/test_gpu_lm_step.py: k_lin_lm -> Schur waves ->
k_cam_assemble -> k_cam_solve -> k_backsub on every launch path; tests/test_gpu_lm_step_kinds.py: the fixed-landmark, pose-only and
landmark-sharded solves).

Path identity and end-of-solve parity cannot see a slightly wrong linear system: LM with a correct gradient reaches the same minimum
with a wrong Hessian.  A solve with max_num_iterations = 1 (2) and num_trim_rounds = 0 does one (two) linearisations, steps and
decisions, its log has one entry per decision and the downloaded window is x0 (+) delta - so the step itself can be compared.

The reference (plain numpy; of the oracle only the probe of the linear problem, Plus() and the problem's cost):
  J        the probe's Jacobian divided by the probe's column scale;  scale: the probe's at x0, kept for the whole solve as in Ceres
  diag     clamp(colnorm^2(J scale), min_lm_diagonal, max_lm_diagonal), D = sqrt(diag / radius)  (asserted equal to the probe's D)
  y        dense least squares of [J scale; diag(D)] y = [r; 0] (Householder QR) with one refinement whose residual and gradient are
           formed in long double;  delta = -y scale;  x1 = Plus(x0, delta) block by block
  scalars  model cost change (J y).(r - J y / 2) in long double, step_norm |x1 - x0| over the state of the reduced program,
           gradient_max_norm max|x - Plus(x, -J^T r)| in ambient space (ceres_like.cpp: NOT max|J^T r|), the costs at x0 and x1 of the
           problem BUILT at x0 (the ground-plane rows and the scale regulariser's constant are fixed when the problem is built),
           relative_decrease, and the radius after the decision by the rule of kba_lm.hpp:lm_decide_step
run_reference() walks Ceres' control flow with these numbers (tolerances, acceptance, radius, termination) and check_step() holds
the output of ANY implementation to it: every parameter block, the log, the report.  The second step after an accepted one is
referenced from a probe AT the implementation's own x1 (its result with max_num_iterations = 1) with the scale of x0 and the radius
the log reports; after a rejected one it is the same J, r with the diagonal reused and the radius halved.

BARS.  One bar per quantity class over all cases: 100 x the largest deviation from this reference that the oracle's Schur-based
solve or the emulator shows on the CPU over all cases of both tiers, rounded up to one digit
(test_lm_step_cpu.py::test_bars_are_100x_the_cpu_spread measures the spread again on every run and fails when it has outgrown a
bar's hundredth by more than a factor of two, or when a bar exceeds 1e-8).  Why 100 x: the GPU differs from those two only by the
summation order inside the MFMA tiles and reductions and by the <= 2 ulp reciprocals of test_gpu_math.py - rounding-level
perturbations that pass through the same conditioning that separates the two CPU implementations from each other - while a wrong
term in a block is at least six digits larger.  Parameter classes are relative to the max-norm of the step over the class, scalars
(log entries, report costs) are relative.  A case whose CPU spread would need a bar above 1e-8 is ill-conditioned input: its seed is
replaced, the bar is not widened.  Never derived from the GPU's own deviation, which is recorded next to them:

    class              CPU spread (emulator / oracle)   bar      MI355X
    landmark           6.4e-12 / 3.4e-12                7e-10    2.4e-12
    pose_rotation      1.2e-11 / 2.1e-11                3e-9     5.7e-12
    pose_translation   1.0e-11 / 1.8e-11                2e-9     5.9e-12
    plane_direction    2.0e-11 / 1.6e-11                2e-9     1.8e-11
    plane_distance     3.9e-12 / 4.5e-12                5e-10    3.3e-12
    scalar             1.7e-12 / 3.3e-12                4e-10    1.2e-12

The same reference serves the other problem kinds (Problem: the probe of tests/cpp/step_kinds_ref.cpp builds the adjustPoseOnly
problem, or the solve() problem with the flagged landmarks constant) and, through check_params_only, the landmark-sharded solve,
which has no log.  The MI355X on those, largest deviation per class (tests/test_gpu_lm_step_kinds.py):

    class              fixed landmarks   pose-only   sharded
    landmark           2.9e-13           -           2.4e-12
    pose_rotation      3.9e-13           2.4e-14     1.7e-12
    pose_translation   6.8e-14           1.1e-13     2.8e-12
    plane_direction    1.8e-11           -           1.7e-11
    plane_distance     1.3e-13           -           3.3e-12
    scalar             1.2e-12           1.7e-13     1.6e-13

(profiles/lm_step_reference.md has the cases behind the maxima.)
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import fixed_lm_common as flc
import iteration_log_common as ilc
import pyoracle
import test_gpu_schur_head as schur_head
from limo_amd import _ffi, default_options, synth
from limo_amd.window import Window

CLASSES = ("landmark", "pose_rotation", "pose_translation", "plane_direction", "plane_distance")
# measured CPU spread (profiles/lm_step_reference.md) x 100, rounded up to one digit
BARS = {
    "landmark": 7e-10,          # CPU spread 6.4e-12 (the emulator's sharded solve, two steps on 12 landmarks over 8 shards)
    "pose_rotation": 3e-9,      # 2.1e-11
    "pose_translation": 2e-9,   # 1.8e-11
    "plane_direction": 2e-9,    # 2.0e-11
    "plane_distance": 5e-10,    # 4.5e-12
    "scalar": 4e-10,            # 3.3e-12
}
MAX_BAR = 1e-8
REPORT_INTS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "num_linearizations", "n_depth_blocks",
               "n_repr_blocks", "n_gp_blocks", "n_trimmed_landmarks")

# ------------------------------------------------------------------------------------------------ shapes and option cases
NEW_SHAPES = [
    dict(seed=7400, n_kf=3, n_lm=120, stereo_baseline=0.5),
    dict(seed=7401, n_kf=2, n_lm=40, depth_prob=1.0),
    dict(seed=7402, n_kf=3, n_lm=100, depth_prob=0, ground_frac=0, with_ground_plane=False),
]
SHAPES = list(schur_head.CASES) + NEW_SHAPES  # the nine windows of the Schur-head test and three more
SMALL = (7102, 7103, 7400, 7401)              # the windows every option case runs on


@functools.lru_cache(maxsize=None)
def _window(seed):
    w = schur_head._window(next(c for c in SHAPES if c["seed"] == seed))
    for name, _ in w.FIELDS:
        getattr(w, name).setflags(write=False)
    return w


def window(seed):
    """A fresh copy of the window of a shape (the cached original is never changed)."""
    return _window(seed).copy()


def step_options(steps=1, **overrides):
    return default_options(num_trim_rounds=0, max_num_iterations=steps, **overrides)


# name -> (option overrides, steps).  Values that have to clamp PART of the columns (min / max_lm_diagonal) are held to that by
# test_lm_step_cpu.py::test_lm_diagonal_cases_clamp_part_of_the_columns, every case to making a difference by
# test_option_cases_are_not_vacuous.
OPTION_CASES = {
    "radius_1e-2": (dict(initial_trust_region_radius=1e-2), 1),
    "radius_1": (dict(initial_trust_region_radius=1.0), 1),
    "radius_1e16": (dict(initial_trust_region_radius=1e16), 1),
    "min_diag": (dict(min_lm_diagonal=0.97), 1),
    "max_diag": (dict(max_lm_diagonal=0.97), 1),
    "min_diag_unscaled": (dict(min_lm_diagonal=1e4, jacobi_scaling=0), 1),
    "max_diag_unscaled": (dict(max_lm_diagonal=1e4, jacobi_scaling=0), 1),
    "loss_scales": (dict(depth_thres=0.5, reprojection_thres=5.0), 1),
    "max_radius_2e4": (dict(max_trust_region_radius=2e4), 2),
    "min_relative_decrease_10": (dict(min_relative_decrease=10.0), 2),
    "gradient_tolerance_1e9": (dict(gradient_tolerance=1e9), 1),
    "min_radius_1e5": (dict(min_trust_region_radius=1e5), 1),
    "parameter_tolerance_1e3": (dict(parameter_tolerance=1e3), 1),
    "function_tolerance_1e3": (dict(function_tolerance=1e3), 1),
    "two_steps": (dict(), 2),
}
SHAPE_CASES = {"default": (dict(), 1), "unscaled": (dict(jacobi_scaling=0), 1)}  # run on all twelve shapes


KIND_CASES = dict(SHAPE_CASES, two_steps_unscaled=(dict(jacobi_scaling=0), 2))  # with OPTION_CASES: what the other problem kinds run
KIND_STEP_CASES = ("default", "unscaled", "two_steps", "two_steps_unscaled")


def all_cases():
    """(case name, seed) of every solve both tiers hold to the reference."""
    out = [(name, c["seed"]) for name in SHAPE_CASES for c in SHAPES]
    return out + [(name, seed) for name in OPTION_CASES for seed in SMALL]


# ---- fixed-landmark windows: the shapes of fixed_lm_common.shapes() but (f), which has nothing to optimise
FIXED_OPTION_CASES = ("radius_1e-2", "min_diag_unscaled", "max_diag_unscaled", "loss_scales", "min_relative_decrease_10", "function_tolerance_1e3")
FIXED_OPTION_WINDOWS = ("a", "b", "e_all", "h_b_02")  # the windows the option cases that constness touches run on


@functools.lru_cache(maxsize=None)
def _fixed_shapes():
    out = flc.shapes()
    for w, flags in out.values():
        flags.setflags(write=False)
        for name, _ in w.FIELDS:
            getattr(w, name).setflags(write=False)
    return out


def fixed_window(name):
    """(a fresh copy of the window, its Problem) of a shape of fixed_lm_common.shapes()."""
    w, flags = _fixed_shapes()[name]
    return w.copy(), Problem(lm_fixed=flags)


def fixed_cases():
    """(case name, shape name): one and - but for the g_* family - two steps, scaled and unscaled, on every shape; the option
    cases on FIXED_OPTION_WINDOWS."""
    names = [n for n in _fixed_shapes() if n != "f"]
    out = [(c, n) for c in KIND_STEP_CASES for n in names if KIND_CASES.get(c, OPTION_CASES.get(c))[1] == 1 or not n.startswith("g_")]
    return out + [(c, n) for c in FIXED_OPTION_CASES for n in FIXED_OPTION_WINDOWS]


# ---- pose-only windows: synth.make_pose_only_case(71..74) with the prior, without one, with speed_weight = 0, and one cut down
POSE_SEEDS = (71, 72, 73, 74)
POSE_OPTION_CASES = ("radius_1", "min_diag", "max_diag", "loss_scales", "min_relative_decrease_10")
# the windows the option cases run on.  min_diag runs on 73 in place of 72: on 72 it clamps one column of six by so little that the
# reference moves by 5e3 bars only, under the 1e4 that test_option_cases_are_not_vacuous asks of every case
POSE_OPTION_WINDOWS = {c: ("71", "73") if c == "min_diag" else ("71", "72") for c in POSE_OPTION_CASES}
POSE_SMALL = "71_small"  # seed 71 cut down to its first 20 landmarks (test_gpu_pose_batch.py's ragged batch), with its prior


@functools.lru_cache(maxsize=None)
def _pose_case(seed):
    w, prior, _ = synth.make_pose_only_case(seed)
    for name, _ in w.FIELDS:
        getattr(w, name).setflags(write=False)
    return w, prior


def _cut_down(w, n_lm):
    sel = w.obs_lm < n_lm
    return Window(kf_pose=w.kf_pose.copy(), kf_plane_dir=w.kf_plane_dir.copy(), kf_plane_dist=w.kf_plane_dist.copy(), kf_fixation=w.kf_fixation.copy(), cam=w.cam.copy(),
                  lm_pos=w.lm_pos[:n_lm].copy(), lm_weight=w.lm_weight[:n_lm].copy(), lm_is_ground=w.lm_is_ground[:n_lm].copy(), obs_kf=w.obs_kf[sel].copy(),
                  obs_lm=w.obs_lm[sel].copy(), obs_cam=w.obs_cam[sel].copy(), obs_u=w.obs_u[sel].copy(), obs_v=w.obs_v[sel].copy(), obs_d=w.obs_d[sel].copy())


def pose_window(name):
    """(a fresh copy of the window, its Problem) of "<seed>" (with its prior), "<seed>_none" (prior = None), "<seed>_w0" (the prior
    with speed_weight = 0: the bits of "<seed>_none") or "<seed>_small" (20 landmarks, with the prior)."""
    seed, _, variant = name.partition("_")
    w, prior = _pose_case(int(seed))
    w = _cut_down(w, 20) if variant == "small" else w.copy()
    if variant == "none":
        return w, Problem("pose_only")
    p = _ffi.SpeedPrior.from_buffer_copy(prior)
    if variant == "w0":
        p.speed_weight = 0.0
    return w, Problem("pose_only", prior=p)


def pose_cases():
    """(case name, window name)."""
    names = [str(s) + v for s in POSE_SEEDS for v in ("", "_none", "_w0")] + [POSE_SMALL]
    return [(c, n) for c in KIND_STEP_CASES for n in names] + [(c, n) for c in POSE_OPTION_CASES for n in POSE_OPTION_WINDOWS[c]]


# ---- landmark-sharded solves: small windows over few and many shards, down to shards that own no landmark
SHARDED_SEEDS = (7102, 7103, 7400, 7401, 7402)
SHARDED_WINDOWS = {"w8": (dict(seed=8, n_kf=2, n_lm=12), (5, 8)), "w9": (dict(seed=9, n_kf=3, n_lm=5), (8,))}  # name -> (make_window arguments, shard counts)


def sharded_window(name):
    """A fresh copy of the window "<seed of SHARDED_SEEDS>" or of a name of SHARDED_WINDOWS."""
    if name in SHARDED_WINDOWS:
        kw = dict(SHARDED_WINDOWS[name][0])
        return synth.make_window(kw.pop("seed"), **kw)
    return window(int(name))


def sharded_cases():
    """(case name, window name, number of shards)."""
    shapes = [(str(s), P) for s in SHARDED_SEEDS for P in (2, 3, 8)] + [(n, P) for n, (_, Ps) in SHARDED_WINDOWS.items() for P in Ps]
    return [(c, n, P) for c in KIND_STEP_CASES for n, P in shapes]


def case_options(name):
    over, steps = KIND_CASES[name] if name in KIND_CASES else OPTION_CASES[name]
    return step_options(steps, **over)


# ------------------------------------------------------------------------------------------------ the problem kinds
class Problem:
    """Which problem a window stands for: kind "solve" (limo_ba_solve; lm_fixed: None, or one flag per landmark, non-zero = a constant
    parameter block - limo_ba_solve_fixed_landmarks) or "pose_only" (limo_ba_adjust_pose_only: n_kf == 1, every landmark constant;
    prior: None or a _ffi.SpeedPrior).  The default is the plain windowed solve, probed through pyoracle as before."""

    def __init__(self, kind="solve", prior=None, lm_fixed=None):
        assert kind in ("solve", "pose_only") and (prior is None or kind == "pose_only") and (lm_fixed is None or kind == "solve")
        self.kind, self.prior = kind, prior
        self.lm_fixed = None if lm_fixed is None else np.ascontiguousarray(np.asarray(lm_fixed).astype(bool).astype(np.uint8))

    @property
    def pose_only(self):
        return self.kind == "pose_only"

    @property
    def plain(self):
        return self.kind == "solve" and self.lm_fixed is None

    def key(self):
        """The bytes of the descriptor (part of the cache key of a linearisation)."""
        return (self.kind, b"" if self.prior is None else bytes(self.prior), b"" if self.lm_fixed is None else self.lm_fixed.tobytes())

    def flags(self, n_lm):
        """The uint8 flags as the libraries take them (at least one byte long), or None."""
        return flc.as_flags(self.lm_fixed, n_lm)


SOLVE = Problem()

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "cpp", "_build")
KINDS_LIB = os.path.join(_BUILD, "libstep_kinds_ref.so")
_kinds = None


def build():
    """tests/cpp/step_kinds_ref.cpp: the probe of every problem kind, with oracle/Makefile's flags (as fixed_lm_common.build)."""
    os.makedirs(_BUILD, exist_ok=True)
    odir = os.path.join(os.path.dirname(_HERE), "oracle")
    src = [os.path.join(_HERE, "cpp", "step_kinds_ref.cpp"), os.path.join(odir, "ceres_like.cpp")]
    deps = src + [os.path.join(_HERE, "cpp", "fixed_lm_ref.cpp")] + [os.path.join(odir, f) for f in ("kba_oracle.cpp", "ceres_like.hpp", "functors.hpp", "jet.hpp")]
    if flc._stale(KINDS_LIB, deps):
        subprocess.check_call(["g++", "-O3", "-march=x86-64-v4", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", KINDS_LIB] + src)


def kinds():
    global _kinds
    if _kinds is None:
        build()
        lib = C.CDLL(KINDS_LIB)
        W, O, P = C.POINTER(_ffi.BaWindow), C.POINTER(_ffi.BaOptions), C.POINTER(_ffi.SpeedPrior)
        dp, ip, u8p, dpp = _ffi.c_double_p, _ffi.c_int32_p, _ffi.c_uint8_p, C.POINTER(_ffi.c_double_p)
        lib.kinds_step_probe.argtypes = [W, O, dpp, C.c_int, P, u8p, ip, dp, dp, dp, dp, dp, ip, dp]
        lib.kinds_problem_cost_at.argtypes = [W, O, dpp, C.c_int, P, u8p, dp]
        lib.kinds_block_counts.argtypes = [W, O, C.c_int, P, ip]
        lib.kinds_last_iteration_log.argtypes = [C.c_int32, C.POINTER(_ffi.BaIteration)]
        lib.ref_ba_solve_fixed.argtypes = [W, u8p, O, C.POINTER(_ffi.BaReport)]
        lib.ref_set_threads.argtypes = [C.c_int]
        lib.ref_set_threads.restype = None
        _kinds = lib
    return _kinds


def _kind_args(w, problem):
    flags = problem.flags(w.n_lm)
    return int(problem.pose_only), (None if problem.prior is None else C.byref(problem.prior)), (None if flags is None else flags.ctypes.data_as(_ffi.c_uint8_p)), flags


def step_probe(w, o, at=None, problem=SOLVE):
    """pyoracle.step_probe for a problem kind (same dict; None when the solve takes no step)."""
    if problem.plain:
        return pyoracle.step_probe(w, o, at)
    lib = kinds()
    s = w.as_struct()
    at4, keep = (None, None) if at is None else pyoracle._at4(w, at)
    po, prior, fl, keep_flags = _kind_args(w, problem)
    sizes = np.zeros(3, np.int32)
    sp = sizes.ctypes.data_as(_ffi.c_int32_p)
    rc = lib.kinds_step_probe(C.byref(s), C.byref(o), at4, po, prior, fl, sp, None, None, None, None, None, None, None)
    if rc == 1:
        return None
    if rc != 0:
        raise RuntimeError("kinds_step_probe rc=%d" % rc)
    m, n = int(sizes[0]), int(sizes[1])
    J, r, D, y, scale, col, costs = np.zeros((m, n)), np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, 3), np.int32), np.zeros(2)
    dp = pyoracle._dp
    rc = lib.kinds_step_probe(C.byref(s), C.byref(o), at4, po, prior, fl, sp, dp(J), dp(r), dp(D), dp(y), dp(scale), col.ctypes.data_as(_ffi.c_int32_p), dp(costs))
    if rc != 0:
        raise RuntimeError("kinds_step_probe rc=%d" % rc)
    return {"J": J, "r": r, "D": D, "y": y, "num_e": int(sizes[2]), "scale": scale, "col": col, "cost": float(costs[0]), "fixed_cost": float(costs[1])}


def problem_cost_at(w, o, at, problem=SOLVE):
    """pyoracle.problem_cost_at for a problem kind: the total cost (constant blocks included) of the problem built at `w`, at `at`."""
    if problem.plain:
        return pyoracle.problem_cost_at(w, o, at)
    s = w.as_struct()
    at4, keep = pyoracle._at4(w, at)
    po, prior, fl, keep_flags = _kind_args(w, problem)
    cost = np.zeros(1)
    rc = kinds().kinds_problem_cost_at(C.byref(s), C.byref(o), at4, po, prior, fl, pyoracle._dp(cost))
    if rc != 0:
        raise RuntimeError("kinds_problem_cost_at rc=%d" % rc)
    return float(cost[0])


def block_counts(w, o, problem=SOLVE):
    """(depth, reprojection, ground-plane) residual blocks of the problem of `w`: the report's n_*_blocks."""
    if problem.plain:
        return [int(c) for c in pyoracle.problem_cost(w, o)[1]]
    s = w.as_struct()
    counts = np.zeros(3, np.int32)
    po, prior, _, _ = _kind_args(w, problem)
    rc = kinds().kinds_block_counts(C.byref(s), C.byref(o), po, prior, counts.ctypes.data_as(_ffi.c_int32_p))
    if rc != 0:
        raise RuntimeError("kinds_block_counts rc=%d" % rc)
    return [int(c) for c in counts]


def oracle_solve_fixed(w, flags, o):
    """ref_ba_solve_fixed of the probe library on `w` IN PLACE: (report, the oracle's iteration table of that solve)."""
    lib = kinds()
    lib.ref_set_threads(1)
    s = w.as_struct()
    rep = _ffi.BaReport()
    rc = lib.ref_ba_solve_fixed(C.byref(s), None if flags is None else flags.ctypes.data_as(_ffi.c_uint8_p), C.byref(o), C.byref(rep))
    if rc != 0:
        raise RuntimeError("ref_ba_solve_fixed rc=%d" % rc)
    n = lib.kinds_last_iteration_log(0, None)
    log = np.zeros(n, _ffi.iteration_dtype())
    if n:
        lib.kinds_last_iteration_log(n, log.ctypes.data_as(C.POINTER(_ffi.BaIteration)))
    return rep.as_dict(), log


# ------------------------------------------------------------------------------------------------ the reference of one step
def _probe_options(o):
    """`o` with the stopping rules that would end the oracle's solve before its first step at their defaults: the probe's J, r,
    scale and D depend on none of them."""
    p = _ffi.BaOptions.from_buffer_copy(o)
    d = default_options()
    p.gradient_tolerance, p.min_trust_region_radius = d.gradient_tolerance, d.min_trust_region_radius
    p.num_trim_rounds, p.max_num_iterations = 0, 1
    return p


def _blocks(col):
    """The parameter blocks of the reduced program: sorted unique (kind, index)."""
    return sorted({(int(k), int(i)) for k, i, _ in col})


def _block(w, kind, index):
    return (w.lm_pos, w.kf_pose, w.kf_plane_dir, w.kf_plane_dist)[kind][index : index + 1].reshape(-1)


def plus(w, col, delta):
    """Plus(x, delta) block by block over the blocks of `col`: a new window."""
    out = w.copy()
    d = {}
    for (k, i, c), v in zip(col, delta):
        d.setdefault((int(k), int(i)), {})[int(c)] = v
    for (k, i), comps in d.items():
        dv = np.array([comps[c] for c in range(len(comps))])
        if k == pyoracle.COL_POSE:
            out.kf_pose[i] = pyoracle.plus(0, w.kf_pose[i], dv)[0]
        elif k == pyoracle.COL_PLANE_DIR:
            out.kf_plane_dir[i] = pyoracle.plus(1, w.kf_plane_dir[i], dv)[0]
        elif k == pyoracle.COL_PLANE_DIST:
            out.kf_plane_dist[i] = w.kf_plane_dist[i] + dv[0]
        else:
            out.lm_pos[i] = w.lm_pos[i] + dv
    return out


def state(w, blocks):
    """The ambient state of the reduced program."""
    return np.concatenate([_block(w, k, i) for k, i in blocks])


def class_parts(w, blocks):
    """name of CLASSES -> the values of that class over the blocks of the reduced program."""
    out = {c: [] for c in CLASSES}
    for k, i in blocks:
        v = _block(w, k, i)
        if k == pyoracle.COL_LANDMARK:
            out["landmark"].append(v)
        elif k == pyoracle.COL_POSE:
            out["pose_rotation"].append(v[:4])
            out["pose_translation"].append(v[4:])
        elif k == pyoracle.COL_PLANE_DIR:
            out["plane_direction"].append(v)
        else:
            out["plane_distance"].append(v)
    return {c: np.concatenate(v) if v else np.zeros(0) for c, v in out.items()}


def same_bytes(a, b):
    return all(getattr(a, n).tobytes() == getattr(b, n).tobytes() for n in ("kf_pose", "kf_plane_dir", "kf_plane_dist", "lm_pos"))


class Linearisation:
    """The linear problem at a point (`at`, or x0 = `w0` itself) of the problem built at w0."""

    def __init__(self, w0, o, at=None, scale=None, problem=SOLVE):
        p = step_probe(w0, _probe_options(o), at, problem)
        assert p is not None, "the oracle takes no step here"
        self.w0, self.o, self.x, self.problem = w0, o, (w0 if at is None else at), problem
        self.col, self.r = p["col"], p["r"]
        self.Ju = p["J"] / p["scale"]
        self.scale = p["scale"] if scale is None else scale  # (iteration 0 fixes the scale of the solve)
        self.Js = self.Ju * self.scale
        self.blocks = _blocks(self.col)
        self.cost_var, self.fixed_cost = p["cost"], p["fixed_cost"]
        self.cost = self.cost_var + self.fixed_cost
        self.diag = np.clip((self.Js**2).sum(0), o.min_lm_diagonal, o.max_lm_diagonal)
        if at is None:  # the probe's own D is that of the first step
            D = np.sqrt(self.diag / o.initial_trust_region_radius)
            assert np.allclose(D, p["D"], rtol=1e-13, atol=0), np.abs(D / p["D"] - 1).max()
        self.probe_y = p["y"] if at is None else None
        # |x - Plus(x, -g)| in ambient space, g = J^T r unscaled
        g = self.Ju.T @ self.r
        proj = plus(self.x, self.col, -g)
        self.gmax = float(np.abs(state(self.x, self.blocks) - state(proj, self.blocks)).max())
        self.x_norm = float(np.linalg.norm(state(self.x, self.blocks)))
        self._qr = {}

    def step(self, radius):
        """The trust-region step at `radius`: dict(y, x1, mcc, step_norm, cand_cost (without the fixed cost), delta)."""
        if radius in self._qr:
            return self._qr[radius]
        D = np.sqrt(self.diag / radius)
        n = len(D)
        A = np.vstack([self.Js, np.diag(D)])
        b = np.r_[self.r, np.zeros(n)]
        Q, R = np.linalg.qr(A)
        y = np.linalg.solve(R, Q.T @ b)
        Al = A.astype(np.longdouble)
        g = Al.T @ (b.astype(np.longdouble) - Al @ y.astype(np.longdouble))  # gradient of the stacked problem at y, long double
        y = y + np.linalg.solve(R, np.linalg.solve(R.T, g.astype(np.float64)))
        Jy = self.Js.astype(np.longdouble) @ y.astype(np.longdouble)
        mcc = float(Jy @ (self.r.astype(np.longdouble) - Jy / 2))
        delta = -y * self.scale
        x1 = plus(self.x, self.col, delta)
        step_norm = float(np.linalg.norm(state(x1, self.blocks) - state(self.x, self.blocks)))
        cand = problem_cost_at(self.w0, self.o, x1, self.problem) - self.fixed_cost
        self._qr[radius] = dict(y=y, x1=x1, mcc=mcc, step_norm=step_norm, cand_cost=cand, delta=delta)
        return self._qr[radius]


_lin_cache = {}


def _opts_key(o):
    return bytes(_probe_options(o))


def linearisation(seed_or_window, o, at=None, scale=None, problem=SOLVE):
    """Cached per (window, problem kind, options that shape the linear problem, point)."""
    w0 = window(seed_or_window) if isinstance(seed_or_window, int) else seed_or_window
    key = (w0.lm_pos.tobytes(), w0.kf_pose.tobytes(), w0.obs_u.tobytes(), w0.obs_kf.tobytes(), w0.kf_fixation.tobytes(), problem.key(), _opts_key(o),
           None if at is None else (at.lm_pos.tobytes(), at.kf_pose.tobytes(), at.kf_plane_dir.tobytes(), at.kf_plane_dist.tobytes()))
    if key not in _lin_cache:
        _lin_cache[key] = Linearisation(w0, o, at, scale, problem)
    return _lin_cache[key]


# ------------------------------------------------------------------------------------------------ Ceres' control flow on the reference
def radius_after_accept(radius, rho, o):
    """kba_lm.hpp:lm_decide_step.  Returns (radius, exact): exact when max() picks 1/3 or the clamp holds with a margin that rounding
    of rho cannot cross - the same IEEE operations then give the same bits."""
    q = 2.0 * rho - 1.0
    f = 1.0 - q * q * q
    new = min(o.max_trust_region_radius, radius / max(1.0 / 3.0, f))
    exact = f < 1.0 / 3.0 - 1e-6 or radius / max(1.0 / 3.0, f) > o.max_trust_region_radius * (1 + 1e-6)
    return new, exact


def run_reference(before, o, mid=None, after=None, problem=SOLVE):
    """Ceres' TrustRegionMinimizer on the reference's numbers for a solve of `before` with at most two iterations.
    mid / after: the implementation's result with max_num_iterations = 1 / its result - the points a relinearisation after an accepted
    step is referenced at; without them the reference's own x1 stands in (the reference alone, test_option_cases_are_not_vacuous).
    Returns dict(entries: expected log - dicts with an extra "radius_exact" and, for an accepted step, "x_ref" (the reference's x1),
    "x_from" (the point stepped from) and "lin" (the linearisation at the implementation's point); termination; ended_in_decision;
    accepted; final_cost; lin0)."""
    assert o.max_num_iterations <= 2 and o.num_trim_rounds == 0
    lin0 = lin = linearisation(before, o, problem=problem)
    radius, dec = o.initial_trust_region_radius, 2.0
    entries = [dict(iteration=0, step_is_valid=1, step_is_successful=1, cost=lin.cost, cost_change=0.0, gradient_max_norm=lin.gmax, step_norm=0.0,
                    relative_decrease=0.0, trust_region_radius=radius, radius_exact=True, model_cost_change=None)]
    it, accepted, ended_in_decision, term = 0, 0, False, None
    while True:
        last = entries[-1]
        if it >= o.max_num_iterations:
            term = _ffi.LIMO_NO_CONVERGENCE
        elif last["step_is_successful"] and lin.gmax <= o.gradient_tolerance:
            term = _ffi.LIMO_CONVERGENCE
        elif radius <= o.min_trust_region_radius:
            term = _ffi.LIMO_CONVERGENCE
        if term is not None:
            break
        it += 1
        s = lin.step(radius)
        assert s["mcc"] > 0.0  # (invalid steps are out of scope: every case takes a valid step)
        if s["step_norm"] <= o.parameter_tolerance * (lin.x_norm + o.parameter_tolerance):
            term, ended_in_decision = _ffi.LIMO_CONVERGENCE, True
            break
        cost_change = lin.cost_var - s["cand_cost"]
        if abs(cost_change) <= o.function_tolerance * lin.cost_var:
            term, ended_in_decision = _ffi.LIMO_CONVERGENCE, True
            break
        rho = cost_change / s["mcc"]
        e = dict(iteration=it, step_is_valid=1, cost=s["cand_cost"] + lin.fixed_cost, cost_change=cost_change, step_norm=s["step_norm"],
                 relative_decrease=rho, model_cost_change=s["mcc"])
        if rho > o.min_relative_decrease:
            accepted += 1
            radius, exact = radius_after_accept(radius, rho, o)
            dec = 2.0
            impl = (after if o.max_num_iterations == it else mid)
            e.update(x_ref=s["x1"], x_from=lin.x)
            lin = linearisation(before, o, at=impl if impl is not None else s["x1"], scale=lin0.scale, problem=problem)
            e.update(step_is_successful=1, gradient_max_norm=lin.gmax, trust_region_radius=radius, radius_exact=exact, lin=lin)
        else:
            radius, dec = radius / dec, dec * 2.0
            e.update(step_is_successful=0, gradient_max_norm=last["gradient_max_norm"], trust_region_radius=radius, radius_exact=True)
        entries.append(e)
    return dict(entries=entries, termination=term, ended_in_decision=ended_in_decision, accepted=accepted, iterations=it,
                final_cost=lin.cost if accepted == 0 else [e for e in entries if e["step_is_successful"]][-1]["cost"], lin0=lin0)


# ------------------------------------------------------------------------------------------------ the check
def _rel(got, want):
    return abs(float(got) - want) / abs(want) if want != 0.0 else abs(float(got))


def _holder(dev, bars, where):
    def hold(cls, value, what):
        dev[cls] = max(dev.get(cls, 0.0), value)
        if bars is not None:
            assert value <= bars[cls], (where, what, cls, "%.3e > %.1e" % (value, bars[cls]))

    return hold


def check_step(before, after, report, log, o, mid=None, counts_ending_iteration=True, bars=BARS, where="", problem=SOLVE):
    """Holds the output of an implementation - the emulator, the oracle, the GPU - for the solve of `before` under `o` (one or two
    iterations, no trimming) to the reference: `after` the window it returned, `report` and `log` its report and iteration log, `mid`
    its result with max_num_iterations = 1 when o allows two.  counts_ending_iteration: iterations_total counts an iteration that ends
    the solve inside the step decision (limo_hip.h; the oracle, like Ceres, does not count it).  bars: None measures only.
    problem: the kind of problem `before` stands for.  Its constant blocks - a flagged landmark, every landmark of a pose-only window,
    a LIMO_FIX_POSE keyframe with its plane - are outside the probe's column map and so have to come back bit for bit; the costs of the
    log and the report include the fixed cost of the residual blocks between constant blocks only, cost_change, relative_decrease and
    the function-tolerance test are formed without it (run_reference).
    Returns the largest deviation per class of BARS (a class without a step in this solve is absent)."""
    ref = run_reference(before, o, mid=mid, after=after, problem=problem)
    want = ref["entries"]
    dev = {}
    hold = _holder(dev, bars, where)

    # --- the log: flags and counts exactly, scalars to the scalar bar
    assert len(log) == len(want), (where, len(log), len(want), [dict(zip(log.dtype.names, e)) for e in log])
    for k, (e, x) in enumerate(zip(log, want)):
        tag = "log[%d]" % k
        assert (int(e["solve"]), int(e["solve_kind"]), int(e["iteration"])) == (0, 2, x["iteration"]), (where, tag)
        assert (int(e["step_is_valid"]), int(e["step_is_successful"])) == (x["step_is_valid"], x["step_is_successful"]), (where, tag, float(e["relative_decrease"]), x["relative_decrease"])
        fields = ["cost", "gradient_max_norm"] if k == 0 else ["cost", "cost_change", "step_norm", "relative_decrease", "gradient_max_norm"]
        for f in fields:
            hold("scalar", _rel(e[f], x[f]), tag + "." + f)
        if k == 0:
            assert e["cost_change"] == 0.0 and e["step_norm"] == 0.0 and e["relative_decrease"] == 0.0, (where, tag)
        else:
            hold("scalar", _rel(float(e["cost_change"]) / float(e["relative_decrease"]), x["model_cost_change"]), tag + ".model_cost_change")
        if x["radius_exact"]:
            assert float(e["trust_region_radius"]) == x["trust_region_radius"], (where, tag, float(e["trust_region_radius"]), x["trust_region_radius"])
        else:
            hold("scalar", _rel(e["trust_region_radius"], x["trust_region_radius"]), tag + ".trust_region_radius")
    _check_report(ref, before, report, o, counts_ending_iteration, problem, hold, where)
    _check_parameters(ref, before, after, mid, o, hold, where)
    return dev


def check_params_only(before, after, report, o, mid=None, log=None, bars=BARS, where="", problem=SOLVE):
    """check_step for an implementation without an iteration log (limo_ba_solve_sharded): the parameters of every step the reference
    accepts against the reference's x1, class by class, the report's costs at the scalar bar and its integers exactly.  log: what
    limo_ctx_last_iteration_log gave after the solve, where the implementation has that reader - no entries (limo_hip.h)."""
    ref = run_reference(before, o, mid=mid, after=after, problem=problem)
    dev = {}
    hold = _holder(dev, bars, where)
    assert log is None or len(log) == 0, (where, len(log))
    _check_report(ref, before, report, o, True, problem, hold, where)
    _check_parameters(ref, before, after, mid, o, hold, where)
    return dev


def check_nothing_to_optimise(before, after, report, log, o, problem, bars=BARS, where=""):
    """A window whose parameter blocks are all constant (limo_hip.h, "Nothing to optimise"): LIMO_CONVERGENCE, zero iterations, no
    log entry, the parameters bit for bit, initial_cost == final_cost == the cost of the problem at the scalar bar.  Returns that
    deviation."""
    assert report["termination"] == _ffi.LIMO_CONVERGENCE, (where, report)
    assert (report["iterations_total"], report["iterations_final"], report["successful_steps"], report["n_trimmed_landmarks"]) == (0, 0, 0, 0), (where, report)
    assert [report[k] for k in ("n_depth_blocks", "n_repr_blocks", "n_gp_blocks")] == block_counts(before, o, problem), (where, report)
    assert len(log) == 0, (where, len(log))
    assert same_bytes(after, before), where
    assert report["initial_cost"] == report["final_cost"], (where, report)
    dev = _rel(report["initial_cost"], problem_cost_at(before, o, before, problem))
    assert bars is None or dev <= bars["scalar"], (where, "%.3e > %.1e" % (dev, bars["scalar"]))
    return dev


def _check_report(ref, before, report, o, counts_ending_iteration, problem, hold, where):
    n_it = ref["iterations"] if (counts_ending_iteration or not ref["ended_in_decision"]) else ref["iterations"] - 1
    counts = block_counts(before, o, problem)
    want_rep = dict(termination=ref["termination"], num_solves=1, iterations_total=n_it, iterations_final=n_it, successful_steps=ref["accepted"],
                    num_linearizations=1 + ref["accepted"], n_depth_blocks=int(counts[0]), n_repr_blocks=int(counts[1]), n_gp_blocks=int(counts[2]),
                    n_trimmed_landmarks=0)
    got_rep = {k: report[k] for k in REPORT_INTS}
    assert got_rep == want_rep, (where, got_rep, want_rep)
    hold("scalar", _rel(report["initial_cost"], ref["entries"][0]["cost"]), "report.initial_cost")
    hold("scalar", _rel(report["final_cost"], ref["final_cost"]), "report.final_cost")


def _check_parameters(ref, before, after, mid, o, hold, where):
    """Every accepted step against the reference's x1 from the point it was taken at, class by class; a solve without one, the
    point after a rejected step and every block outside the reduced program bit for bit."""
    want = ref["entries"]
    points = {1: mid if o.max_num_iterations == 2 else after, 2: after}
    cur = before
    blocks = ref["lin0"].blocks
    for x in want[1:]:
        if not x["step_is_successful"]:
            continue
        got = points[x["iteration"]]
        assert got is not None, "mid: the implementation's result with max_num_iterations = 1"
        a, b, c = class_parts(x["x_from"], blocks), class_parts(x["x_ref"], blocks), class_parts(got, blocks)
        for cls in CLASSES:
            step = np.abs(b[cls] - a[cls]).max() if len(a[cls]) else 0.0
            if step == 0.0:  # the class is not in the problem
                assert c[cls].tobytes() == a[cls].tobytes(), (where, cls)
                continue
            hold(cls, float(np.abs(c[cls] - b[cls]).max() / step), "step %d" % x["iteration"])
        cur = got
    if cur is before:  # no accepted step: the parameters are the input, bit for bit
        assert same_bytes(after, before), where
        assert mid is None or same_bytes(mid, before), where
    elif want[-1]["step_is_successful"] == 0:  # accepted, then rejected
        assert same_bytes(after, cur), where
    # blocks outside the reduced program never move
    inside = set(blocks)
    for kind, n in ((0, before.n_lm), (1, before.n_kf), (2, before.n_kf), (3, before.n_kf)):
        for i in range(n):
            if (kind, i) not in inside:
                assert _block(after, kind, i).tobytes() == _block(before, kind, i).tobytes(), (where, kind, i)


def merge(total, dev):
    for k, v in dev.items():
        total[k] = max(total.get(k, 0.0), v)
    return total


# ------------------------------------------------------------------------------------------------ the two CPU implementations
def emu_run(seeds, o, problem=SOLVE):
    """The emulator on the windows of `seeds` (seeds of SHAPES, or windows: all of the kind `problem`) under `o`:
    [(before, after, report, log)]."""
    before = [window(s) if isinstance(s, int) else s.copy() for s in seeds]
    after = [w.copy() for w in before]
    flags = None if problem.lm_fixed is None else [problem.flags(w.n_lm) for w in after]
    reps, logs = ilc.emu_solve(after, o, pose_only=problem.pose_only, prior=problem.prior, lm_fixed=flags)
    return list(zip(before, after, reps, logs))


def oracle_run(seed, o, problem=SOLVE):
    """The oracle's own solve of the problem kind on a window (a seed of SHAPES, or a window): (before, after, report, its table)."""
    before = window(seed) if isinstance(seed, int) else seed.copy()
    after = before.copy()
    if problem.pose_only:
        rep = pyoracle.adjust_pose_only(after, problem.prior, o)
    elif problem.lm_fixed is not None:
        rep, log = oracle_solve_fixed(after, problem.flags(after.n_lm), o)
        return before, after, rep, log
    else:
        rep, _ = pyoracle.solve(after, o)
    return before, after, rep, pyoracle.last_iteration_log()


def emu_run_sharded(w, o, n_shards):
    """The emulator's landmark-sharded solve (virtual shards) of a window: (before, after, report) - it has no log."""
    import emu_ffi

    after = w.copy()
    rep = emu_ffi.solve_sharded(after, o, n_shards)
    return w, after, rep


def one_step_options(o):
    p = _ffi.BaOptions.from_buffer_copy(o)
    p.max_num_iterations = 1
    return p


def reference_difference(seed, o_a, o_b, problem=SOLVE, problem_b=None):
    """How far the references of one window (a seed of SHAPES, or a window of the kind `problem`) under two option sets - and, with
    problem_b, two descriptors of the same blocks - are apart: inf when the expected flow differs (entries, flags, termination), else
    the largest relative difference of a logged scalar or a parameter class, each divided by its bar."""
    before = window(seed) if isinstance(seed, int) else seed
    ra, rb = run_reference(before, o_a, problem=problem), run_reference(before, o_b, problem=problem if problem_b is None else problem_b)
    ka = [(e["iteration"], e["step_is_valid"], e["step_is_successful"]) for e in ra["entries"]]
    kb = [(e["iteration"], e["step_is_valid"], e["step_is_successful"]) for e in rb["entries"]]
    if ka != kb or ra["termination"] != rb["termination"] or ra["ended_in_decision"] != rb["ended_in_decision"]:
        return float("inf")
    worst = 0.0
    blocks = ra["lin0"].blocks
    for ea, eb in zip(ra["entries"], rb["entries"]):
        for f in ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius"):
            worst = max(worst, _rel(ea[f], eb[f]) / BARS["scalar"] if eb[f] != 0.0 else 0.0)
        if "x_ref" in ea and "x_ref" in eb:
            a, b, x0 = class_parts(ea["x_ref"], blocks), class_parts(eb["x_ref"], blocks), class_parts(ea["x_from"], blocks)
            for cls in CLASSES:
                step = np.abs(b[cls] - x0[cls]).max() if len(b[cls]) else 0.0
                if step > 0.0:
                    worst = max(worst, float(np.abs(a[cls] - b[cls]).max() / step) / BARS[cls])
    return worst
