"""Inputs shared by tests/test_gpu_window_options.py (per-window solve options, limo_ba_batch_solve_each): the windows, the options
drawn per window, and the check that the inputs CAN tell - a window whose options differ from entry 0's must come out differently
under them (oracle, CPU).  Test infrastructure."""
import functools

import numpy as np

from limo_amd import default_options, synth

# (seed, make_window keywords): the smallest shapes at which the table read can go wrong -
#   n_lm 40: no trimming (<= 100), only the thresholds act;  n_lm 130 / 300: trimming runs, the quantiles decide;
#   7 keyframes: the generic Schur class (k_schur_wide);  stereo_baseline > 0: two views per keyframe.
SHAPES = (
    (401, dict(n_kf=3, n_lm=40)),
    (402, dict(n_kf=5, n_lm=40)),
    (403, dict(n_kf=3, n_lm=130)),
    (404, dict(n_kf=5, n_lm=130)),
    (405, dict(n_kf=3, n_lm=300)),
    (406, dict(n_kf=5, n_lm=300)),
    (407, dict(n_kf=7, n_lm=130)),
    (408, dict(n_kf=4, n_lm=130, stereo_baseline=0.54)),
    (409, dict(n_kf=5, n_lm=300)),
    (410, dict(n_kf=3, n_lm=40)),
    (411, dict(n_kf=4, n_lm=300)),
    (412, dict(n_kf=5, n_lm=130)),
)
# (depth_thres, reprojection_thres, depth_quantile, reprojection_quantile) per window, from {0.08, 0.16, 0.4} x {0.8, 1.6, 3.0} x
# {0.8, 0.95, 1.0}; windows 8 and 9 share entry 0's.  The windows that do not trim differ from entry 0 in a threshold.
DRAWN = (
    (0.16, 1.6, 0.95, 0.95),
    (0.08, 3.0, 0.8, 1.0),
    (0.4, 1.6, 0.8, 0.95),
    (0.16, 0.8, 0.95, 0.8),
    (0.08, 0.8, 1.0, 0.8),
    (0.4, 3.0, 0.8, 0.8),
    (0.08, 1.6, 0.8, 0.95),
    (0.4, 0.8, 0.95, 0.8),
    (0.16, 1.6, 0.95, 0.95),
    (0.16, 1.6, 0.95, 0.95),
    (0.16, 3.0, 1.0, 1.0),
    (0.16, 1.6, 0.8, 0.8),
)
COOP_SUBSET = tuple(i for i, (_, kw) in enumerate(SHAPES) if kw["n_kf"] <= 5 and not kw.get("stereo_baseline"))  # <= 4 free keyframes, one camera


def options(drawn, **common):
    d, r, qd, qr = drawn
    return default_options(depth_thres=d, reprojection_thres=r, depth_quantile=qd, reprojection_quantile=qr, **common)


@functools.lru_cache(maxsize=None)
def windows():
    return tuple(synth.make_window(seed, **kw) for seed, kw in SHAPES)


def window_options():
    return [options(d) for d in DRAWN]


def same_options(i, j=0):
    return DRAWN[i] == DRAWN[j]


def differs(ra, ta, rb, tb):
    """Two results of one window tell their options apart: in the trimmed set or in the final cost."""
    return (not np.array_equal(np.sort(ta), np.sort(tb))) or ra["final_cost"] != rb["final_cost"]


def oracle_tells_apart():
    """Per window whose options differ from entry 0's: does the oracle's result under its own options differ from its result under
    entry 0's?  (What is run on the CPU before the choice of seeds is trusted with a GPU run.)"""
    import pyoracle

    out = {}
    o0 = window_options()[0]
    for i, (w, o) in enumerate(zip(windows(), window_options())):
        if same_options(i):
            continue
        a, b = w.copy(), w.copy()
        ra, _ = pyoracle.solve(a, o)
        ta = pyoracle.last_trimmed()
        rb, _ = pyoracle.solve(b, o0)
        tb = pyoracle.last_trimmed()
        out[i] = differs(ra, ta, rb, tb)
    return out
