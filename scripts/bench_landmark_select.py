"""Landmark selection: limo_landmark_select / limo_landmark_select_batch (the device) against the host selector in the SAME run
(include/limo_hip.h; the host selector - LandmarkSelector with cheirality + voxel + add-depth as StreamDriver wires them - through
tests/cpp/landmark_select_ref.cpp, timed around LandmarkSelector::select alone: the objects are built before).

For n_lm in --sizes landmarks and n_kf in --windows keyframes (tests/landmark_select_common.make_pool, the node's parameters and its
must-have list for a window of that size), in one process on one GPU, after --warmup calls, median of --reps calls:
  host        LandmarkSelector::select, one CPU thread
  device      limo_landmark_select, host to host: validation, packing, upload, three kernels, the bytes back
  kernels     the device time of the three kernels of that call (HIP events on the context's stream)
  batch N     limo_landmark_select_batch over N pools of that shape (N in --batches), per pool, against N host selections
Both go through ctypes with the arrays made beforehand.  Every device result is compared with the host's bytes.  Prints a table and one
JSON document (--out FILE)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import landmark_select_common as lsc  # noqa: E402
from limo_amd import _ffi, ba  # noqa: E402


def median_ms(f, warmup, reps):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1500,4000")
    ap.add_argument("--windows", default="5,12")
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = ba.Context(0)
    ctx.set_select_timing(True)
    lib, ref = ctx.lib, lsc.ref_lib()
    rows = []
    for n_lm in [int(s) for s in a.sizes.split(",")]:
        for n_kf in [int(s) for s in a.windows.split(",")]:
            # the node's wiring (sequence.hpp: configureSequence): budgets 200 / 200 / 100, the 50 nearest ground landmarks of every keyframe of the window
            p = lsc.params(add=[(i, 50, _ffi.SELECT_IS_GROUND, _ffi.SELECT_KEY_RANGE) for i in range(n_kf)])
            pool = lsc.make_pool(n_lm + n_kf, n_lm, n_kf)
            w, keep = _ffi.select_pool(pool)
            out_d, out_h = np.zeros(n_lm, np.uint8), np.zeros(n_lm, np.uint8)
            sec, host_s, kern = C.c_double(0.0), [], []

            def host():
                assert ref.landmark_select_ref(C.byref(w), C.byref(p), out_h.ctypes.data_as(_ffi.c_uint8_p), C.byref(sec), 0) == 0
                host_s.append(sec.value)

            def device():
                rc = lib.limo_landmark_select(ctx.ptr, C.byref(w), C.byref(p), out_d.ctypes.data_as(_ffi.c_uint8_p))
                if rc != 0:
                    raise ba.LimoError("limo_landmark_select rc=%d %s" % (rc, lib.limo_last_error(ctx.ptr)))
                kern.append(ctx.select_kernel_ms())

            median_ms(host, a.warmup, a.reps)
            t_host = 1e3 * statistics.median(host_s[a.warmup:])
            t_dev = median_ms(device, a.warmup, a.reps)
            t_kern = statistics.median(kern[a.warmup:])
            row = {"n_lm": n_lm, "n_kf": n_kf, "n_obs": int(w.n_obs), "selected": int((out_h & 7 != 0).sum()), "host_ms": t_host, "device_ms": t_dev, "kernels_ms": t_kern,
                   "device_over_host": t_dev / t_host, "same_bytes": bool(out_d.tobytes() == out_h.tobytes()), "batch": []}
            print("n_lm %5d n_kf %2d (%6d obs, %3d selected): host %7.3f ms | device %7.3f ms (kernels %6.3f) x%.2f of the host | same bytes: %s" % (
                n_lm, n_kf, w.n_obs, row["selected"], t_host, t_dev, t_kern, row["device_over_host"], row["same_bytes"]), flush=True)
            for nb in [int(s) for s in a.batches.split(",")]:
                pools = [lsc.make_pool(7000 + 13 * i + n_lm + n_kf, n_lm, n_kf) for i in range(nb)]
                packed = [_ffi.select_pool(q) for q in pools]
                arr = (_ffi.SelectPool * nb)(*[q[0] for q in packed])
                outs = [np.zeros(n_lm, np.uint8) for _ in range(nb)]
                ptrs = (_ffi.c_uint8_p * nb)(*[o.ctypes.data_as(_ffi.c_uint8_p) for o in outs])
                want = np.zeros(n_lm, np.uint8)
                kb = []

                def batch():
                    rc = lib.limo_landmark_select_batch(ctx.ptr, nb, arr, C.byref(p), ptrs)
                    if rc != 0:
                        raise ba.LimoError("limo_landmark_select_batch rc=%d %s" % (rc, lib.limo_last_error(ctx.ptr)))
                    kb.append(ctx.select_kernel_ms())

                reps = a.reps if nb <= 16 else max(5, a.reps // 4)
                t_b = median_ms(batch, min(a.warmup, 2), reps)
                same, t_h = True, 0.0
                for i in range(nb):  # the host selector on every pool of the batch, once
                    assert ref.landmark_select_ref(C.byref(arr[i]), C.byref(p), want.ctypes.data_as(_ffi.c_uint8_p), C.byref(sec), 0) == 0
                    t_h += 1e3 * sec.value
                    same = same and want.tobytes() == outs[i].tobytes()
                b = {"pools": nb, "batch_ms": t_b, "per_pool_ms": t_b / nb, "kernels_ms": statistics.median(kb), "host_ms": t_h, "host_per_pool_ms": t_h / nb,
                     "batch_over_host": t_b / t_h, "same_bytes": bool(same)}
                row["batch"].append(b)
                print("    batch of %3d: %8.3f ms = %7.3f ms per pool (kernels %7.3f ms) | host %8.3f ms = %7.3f per pool | x%.2f of the host | same bytes: %s" % (
                    nb, t_b, t_b / nb, b["kernels_ms"], t_h, t_h / nb, b["batch_over_host"], same), flush=True)
                del packed
            rows.append(row)
            del keep
    doc = {"what": "landmark selection: limo_landmark_select[_batch] vs LandmarkSelector::select on one CPU thread, same run; median of %d calls after %d warm-ups" % (a.reps, a.warmup),
           "pools": "tests/landmark_select_common.make_pool; the node's parameters, 50 ground must-haves per keyframe of the window", "cpus": os.cpu_count(), "cpus_usable": len(os.sched_getaffinity(0)), "rows": rows}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
