"""Kernel time of a batch of windows with constant landmarks (include/limo_hip.h: limo_ba_batch_create_fixed_landmarks).

N C2 windows (5 keyframes, 2000 landmarks; --windows, default 1024) in one process on one GPU, with 0 %, 50 % and 100 % of every
window's landmarks flagged constant (index % 2 == 0 at 50 %): reset + solve per repetition through the streaming solve with ONE
slot group (KBA_GROUPS=1: limo_ba_batch_kernel_time only times kernels that do not overlap), and per fraction the device time per
launch of the linearisation (k_lin_lm) and of the Schur kernels, the number of launches, and the whole solve.  The 0 % batch is
made twice - by limo_ba_batch_create and with all-zero flags - and has to give the same bits.  Prints a table and one JSON
document (--out FILE).
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from limo_amd import ba, default_options, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64, help="distinct synthetic windows (seeds 7000..), cycled over the batch")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["KBA_GROUPS"] = "1"
    os.environ["KBA_STREAM_MIN"] = "1"
    ctx = ba.Context(0)
    o = default_options()
    base = [synth.make_window(7000 + i, n_kf=5, n_lm=2000) for i in range(min(a.distinct, a.windows))]
    wins = [base[i % len(base)].copy() for i in range(a.windows)]
    rows = []
    for label, frac in (("0 % (limo_ba_batch_create)", None), ("0 % (all-zero flags)", 0.0), ("50 %", 0.5), ("100 %", 1.0)):
        flags = None if frac is None else [((np.arange(w.n_lm) % 2 == 0) if frac == 0.5 else np.full(w.n_lm, frac == 1.0)).astype(np.uint8) for w in wins]
        b = ba.Batch(ctx, [w.copy() for w in wins], lm_fixed=flags)  # (download writes into the batch's own copies)
        b.solve(o)  # warm-up (streams, events, worklists)
        path = ctx.last_solve_info()["path"]
        ms = []
        b.kernel_stats(reset=True)
        for _ in range(a.reps):
            b.reset()
            t0 = time.perf_counter()
            b.solve(o)
            ms.append((time.perf_counter() - t0) * 1e3)
        st = b.kernel_stats()
        reps = b.download()
        h = hashlib.sha256()
        for w in b.windows:
            h.update(w.kf_pose.tobytes())
            h.update(w.lm_pos.tobytes())
        b.close()
        rows.append({
            "constant": label, "path": path, "windows": a.windows, "solve_ms_median": statistics.median(ms),
            "linearize_launches": st["linearize_launches"] // a.reps, "linearize_us_per_launch": 1e3 * st["linearize_ms"] / max(1, st["linearize_launches"]),
            "schur_launches": st["schur_launches"] // a.reps, "schur_us_per_launch": 1e3 * st["schur_ms"] / max(1, st["schur_launches"]),
            "lm_iterations": int(sum(r["iterations_total"] for r in reps)), "sha256": h.hexdigest()[:16]})
        r = rows[-1]
        print("%-28s %-9s solve %8.2f ms | k_lin_lm %5d launches, %7.1f us each | Schur %5d launches, %7.1f us each | %7d LM iterations | %s"
              % (label, path, r["solve_ms_median"], r["linearize_launches"], r["linearize_us_per_launch"], r["schur_launches"], r["schur_us_per_launch"],
                 r["lm_iterations"], r["sha256"]), flush=True)
    assert rows[0]["sha256"] == rows[1]["sha256"], "all-zero flags changed the result"
    assert rows[3]["schur_launches"] == 0
    doc = {"script": "scripts/gpu_fixed_landmarks.py", "rows": rows}
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
