"""What the per-window options table costs (limo_ba_batch_solve_each): the same N C2 windows, resident, solved with one set of options
(no table: the kernels see a null pointer) and with N different sets (thresholds from tune_parameters_kitti.py's grid around the
defaults, both quantiles 0.95), alternated, reset + solve timed.  The two solves do different work - other thresholds, other
iteration counts - so the iterations are printed next to the times, and a third solve isolates the table: N entries with the uniform
values, one of them moved by one ulp (the table is read by every workgroup, the work is the uniform solve's).
usage: python scripts/gpu_window_options_cost.py [N = 1024] [repeats = 5]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
from limo_amd import ba, default_options, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ctx = ba.Context(0)
uniform = default_options()
each = [default_options(depth_thres=0.04 * (1 + i % 10), reprojection_thres=0.4 * (1 + (i // 10) % 11)) for i in range(n)]
import numpy as np

same = [default_options() for _ in range(n)]
same[n - 1].reprojection_thres = float(np.nextafter(1.6, 2.0))
b = ba.Batch(ctx, [synth.config_c2(2000 + i) for i in range(n)])
times, iters = {"uniform": [], "table": [], "each": []}, {}
for r in range(reps + 1):
    for name, o in (("uniform", uniform), ("table", same), ("each", each)):
        b.reset()
        t0 = time.perf_counter()
        b.solve(o)
        dt = time.perf_counter() - t0
        if r:  # (the first round warms up)
            times[name].append(dt)
        else:
            iters[name] = sum(rep["iterations_total"] for rep in b.download())
        path = ctx.last_solve_info()["path"]
b.close()
mu, me, mt = statistics.median(times["uniform"]), statistics.median(times["each"]), statistics.median(times["table"])
print("%d C2 windows, the table with the uniform values (one entry one ulp off): %.2f ms (%d LM iterations), ratio to uniform %.3f" % (n, 1e3 * mt, iters["table"], mt / mu))
print("%d C2 windows on the %s path, reset + solve, median of %d: uniform %.2f ms (%d LM iterations) | %d option sets %.2f ms (%d LM iterations) | ratio %.3f, per LM iteration %.3f" % (
    n, path, reps, 1e3 * mu, iters["uniform"], n, 1e3 * me, iters["each"], me / mu, (me / iters["each"]) / (mu / iters["uniform"])))
print("  uniform runs, ms: %s" % " ".join("%.2f" % (1e3 * t) for t in times["uniform"]))
print("  table runs, ms:   %s" % " ".join("%.2f" % (1e3 * t) for t in times["table"]))
print("  each runs, ms:    %s" % " ".join("%.2f" % (1e3 * t) for t in times["each"]))
