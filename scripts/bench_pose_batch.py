"""Batched pose-only adjustment against N single calls (include/limo_hip.h: limo_ba_adjust_pose_only_batch).

For N windows of the make_pose_only_case shape (one keyframe, 300 landmarks, ~300 observations; a prior on every second window), in
one process on one GPU, after a warm-up, median of --reps repetitions:
  singles   N calls of limo_ba_adjust_pose_only (the only way to do this before the batched entry points)
  batch     ONE call of limo_ba_adjust_pose_only_batch
  resident  limo_ba_batch_solve alone on a batch made once by limo_ba_batch_create_pose_only (reset outside the clock)
All three go through the C-ABI with the limo_ba_window structs made beforehand (what a C / C++ caller holds anyway); the poses are
put back to their initial values before every repetition, outside the clock.  Prints a table and one JSON document (--out FILE).
KBA_HOST_TRACE=1 in the environment makes the library print where the host time of every call goes.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from limo_amd import _ffi, ba, default_options, synth  # noqa: E402
from limo_amd.window import struct_array  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64,256,1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", type=int, default=64, help="distinct synthetic cases (seeds 71..), cycled over the windows of a batch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    ctx = ba.Context(0)
    lib = ctx.lib
    o = default_options(min_landmarks_for_trimming=30)
    cases = [synth.make_pose_only_case(71 + i)[:2] for i in range(min(a.cases, max(sizes)))]
    rows = []
    for n in sizes:
        wins = [cases[i % len(cases)][0].copy() for i in range(n)]
        pose0 = [w.kf_pose.copy() for w in wins]
        prior_list = [cases[i % len(cases)][1] if i % 2 == 0 else None for i in range(n)]
        priors = ba.prior_array(prior_list, n)
        arr = struct_array(wins)
        reps = (_ffi.BaReport * n)()

        def restore():
            for w, p in zip(wins, pose0):
                w.kf_pose[:] = p

        def singles():
            for i in range(n):
                rc = lib.limo_ba_adjust_pose_only(ctx.ptr, C.byref(arr[i]), C.byref(priors[i]) if prior_list[i] is not None else None, C.byref(o), C.byref(reps[i]))
                if rc != 0:
                    raise ba.LimoError("limo_ba_adjust_pose_only rc=%d" % rc)

        def batch():
            rc = lib.limo_ba_adjust_pose_only_batch(ctx.ptr, n, arr, priors, C.byref(o), reps)
            if rc != 0:
                raise ba.LimoError("limo_ba_adjust_pose_only_batch rc=%d" % rc)

        def timed(f):
            ts = []
            for r in range(a.reps + 1):  # (the first one warms up)
                restore()
                t0 = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts[1:])

        t_single = timed(singles)
        ref = [(w.kf_pose.tobytes(), reps[i].final_cost, reps[i].iterations_total) for i, w in enumerate(wins)]
        t_batch = timed(batch)
        same = all(ref[i] == (w.kf_pose.tobytes(), reps[i].final_cost, reps[i].iterations_total) for i, w in enumerate(wins))
        restore()
        b = ba.Batch(ctx, wins, arr=arr, pose_only=True, priors=prior_list)
        ts = []
        b.kernel_stats(reset=True)
        for r in range(a.reps + 1):
            b.reset()
            t0 = time.perf_counter()
            b.solve(o)
            ts.append(time.perf_counter() - t0)
        t_res = statistics.median(ts[1:])
        dev_ms = b.kernel_stats()["total_ms"] / (a.reps + 1)
        b.close()
        restore()
        row = {"n_windows": n, "singles_ms": t_single * 1e3, "batch_ms": t_batch * 1e3, "resident_solve_ms": t_res * 1e3, "resident_device_ms": dev_ms,
               "singles_us_per_window": t_single * 1e6 / n, "batch_us_per_window": t_batch * 1e6 / n, "resident_us_per_window": t_res * 1e6 / n,
               "speedup_batch_vs_singles": t_single / t_batch, "batch_bit_identical_to_singles": bool(same)}
        rows.append(row)
        print("N = %5d: singles %9.3f ms (%7.1f us/window) | batch %9.3f ms (%7.1f us/window, x%.2f) | resident solve %8.3f ms (%6.2f us/window, device %.3f ms) | same bits: %s" % (
            n, row["singles_ms"], row["singles_us_per_window"], row["batch_ms"], row["batch_us_per_window"], row["speedup_batch_vs_singles"],
            row["resident_solve_ms"], row["resident_us_per_window"], dev_ms, same), flush=True)
    doc = {"what": "pose-only adjustment: one batched call vs N single calls, median of %d repetitions after one warm-up" % a.reps,
           "window_shape": "synth.make_pose_only_case: 1 keyframe, 300 landmarks, prior on every second window, min_landmarks_for_trimming=30",
           "rows": rows}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
