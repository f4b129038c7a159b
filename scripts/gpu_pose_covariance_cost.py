"""What the marginal pose covariance costs: a resident batch of C2 windows (step = reset + solve), the single
limo_ba_solve call and the single adjustPoseOnly call, each with the context's switch off and on.  Prints one JSON line.
LIMO_HIP_LIB=<another build of the library> measures that build (a build without the switch reports the "off" figures only)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from limo_amd import _ffi, ba, default_options, synth  # noqa: E402


def _time(fn, reps):
    fn()
    best = float("inf")
    for _ in range(3):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        best = min(best, (time.perf_counter() - t) / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = ba.Context(0)
    o = default_options()
    has = hasattr(ctx.lib, "limo_ctx_set_pose_covariance")
    out = {"lib": _ffi.LIB_PATH, "has_switch": has, "batch": a.batch}
    distinct = [synth.config_c2(seed=2 + i) for i in range(min(64, a.batch))]
    windows = [distinct[i % len(distinct)] for i in range(a.batch)]
    single = synth.config_c2()
    wp, prior, _ = synth.make_pose_only_case(71)
    for on in ((False, True) if has else (False,)):
        if has:
            ctx.set_pose_covariance(on)
        b = ba.Batch(ctx, [w.copy() for w in windows])

        def step():
            b.reset()
            b.solve(o)

        key = "on" if on else "off"
        out["batch_solves_per_s_" + key] = a.batch / _time(step, a.reps)
        b.close()
        out["single_solve_ms_" + key] = 1e3 * _time(lambda: ctx.solve(single.copy(), o), 20)
        out["pose_only_ms_" + key] = 1e3 * _time(lambda: ctx.adjust_pose_only(wp.copy(), prior, o), 50)
    if has:
        ctx.set_pose_covariance(False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
