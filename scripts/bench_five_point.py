"""Five-point motion prior: limo_five_point (the device) against the host estimator limo_amd/kba/five_point.hpp in the SAME run
(include/limo_hip.h: limo_five_point / limo_five_point_batch; the host estimator through tests/cpp/five_point_ref.cpp).

For n in --sizes matches and every outlier share in --shares (0.3 px noise, forward motion, tests/five_point_common.make_matches), in
one process on one GPU, after --warmup calls, median of --reps calls:
  host     five_point::estimateMotion, one CPU thread (one sample after the other, early-abandoned counts)
  device   limo_five_point with the library's chunk schedule
and for --batch frames of one (n, share): limo_five_point_batch against that many single calls.  Both go through ctypes with the
arrays made beforehand.  Every device result is compared with the host's bytes.  Prints a table and one JSON document (--out FILE).
"""
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
import five_point_common as fpc  # noqa: E402
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
    ap.add_argument("--sizes", default="300,1500")
    ap.add_argument("--shares", default="0.1,0.3,0.5,0.6")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = ba.Context(0)
    lib, ref = ctx.lib, fpc.ref_lib()
    prm = ctx.five_point_params(chunk=a.chunk)
    rows = []
    dp = _ffi.c_double_p

    def frame(pa, pb, seed):
        return _ffi.FivePointFrame(len(pa), pa.ctypes.data_as(dp), pb.ctypes.data_as(dp), seed)

    for n in [int(s) for s in a.sizes.split(",")]:
        for share in [float(s) for s in a.shares.split(",")]:
            seed = 7
            pa, pb = fpc.make_matches(int(100 * share) + n, n, share)
            fr = frame(pa, pb, seed)
            m_dev, m_host = _ffi.FivePointMotion(), _ffi.FivePointMotion()

            def host():
                rc = ref.five_point_ref_estimate(n, fr.pts_a, fr.pts_b, fpc.FOCAL, fpc.CX, fpc.CY, prm.probability, prm.threshold_px, seed, prm.max_samples,
                                                 C.byref(m_host), None)
                assert rc == 0

            def device():
                rc = lib.limo_five_point(ctx.ptr, C.byref(fr), fpc.FOCAL, fpc.CX, fpc.CY, C.byref(prm), C.byref(m_dev), None)
                if rc != 0:
                    raise ba.LimoError("limo_five_point rc=%d %s" % (rc, lib.limo_last_error(ctx.ptr)))

            t_host = median_ms(host, a.warmup, a.reps)
            t_dev = median_ms(device, a.warmup, a.reps)
            same = bytes(m_dev) == bytes(m_host)
            row = {"matches": n, "outlier_share": share, "samples": int(m_host.samples), "inliers": int(m_host.inliers), "host_ms": t_host, "device_ms": t_dev,
                   "device_over_host": t_dev / t_host, "same_bits": bool(same)}
            rows.append(row)
            print("n = %4d share %.1f: %4d samples, %4d inliers | host %8.3f ms | device %8.3f ms (x%.2f of the host) | same bits: %s" % (
                n, share, row["samples"], row["inliers"], t_host, t_dev, row["device_over_host"], same), flush=True)
    batch_rows = []
    for n, share in ((300, 0.3), (1500, 0.3), (1500, 0.5)):
        keep = [fpc.make_matches(900 + i, n, share) for i in range(a.batch)]
        frames = (_ffi.FivePointFrame * a.batch)(*[frame(pa, pb, 30 + i) for i, (pa, pb) in enumerate(keep)])
        ms_b, ms_s = (_ffi.FivePointMotion * a.batch)(), (_ffi.FivePointMotion * a.batch)()

        def batch():
            rc = lib.limo_five_point_batch(ctx.ptr, a.batch, frames, fpc.FOCAL, fpc.CX, fpc.CY, C.byref(prm), ms_b)
            if rc != 0:
                raise ba.LimoError("limo_five_point_batch rc=%d" % rc)

        def singles():
            for i in range(a.batch):
                rc = lib.limo_five_point(ctx.ptr, C.byref(frames[i]), fpc.FOCAL, fpc.CX, fpc.CY, C.byref(prm), C.byref(ms_s[i]), None)
                if rc != 0:
                    raise ba.LimoError("limo_five_point rc=%d" % rc)

        def hosts():
            m = _ffi.FivePointMotion()
            for i in range(a.batch):
                ref.five_point_ref_estimate(n, frames[i].pts_a, frames[i].pts_b, fpc.FOCAL, fpc.CX, fpc.CY, prm.probability, prm.threshold_px, 30 + i,
                                            prm.max_samples, C.byref(m), None)

        t_b, t_s, t_h = median_ms(batch, a.warmup, a.reps), median_ms(singles, a.warmup, a.reps), median_ms(hosts, 1, max(3, a.reps // 4))
        same = bytes(ms_b) == bytes(ms_s)
        row = {"frames": a.batch, "matches": n, "outlier_share": share, "samples": [int(m.samples) for m in ms_b], "batch_ms": t_b, "singles_ms": t_s, "host_ms": t_h,
               "speedup_batch_vs_singles": t_s / t_b, "batch_bit_identical_to_singles": bool(same)}
        batch_rows.append(row)
        print("%d frames, n = %d, share %.1f: batch %8.3f ms | singles %8.3f ms (x%.2f) | host %8.3f ms | same bits: %s" % (
            a.batch, n, share, t_b, t_s, t_s / t_b, t_h, same), flush=True)
    doc = {"what": "five-point motion prior: limo_five_point vs five_point::estimateMotion on one CPU thread, same run; median of %d calls after %d warm-ups" % (a.reps, a.warmup),
           "matches": "tests/five_point_common.make_matches: forward motion, 0.3 px noise, gross outliers anywhere in the image", "chunk": a.chunk,
           "rows": rows, "batch_rows": batch_rows}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
