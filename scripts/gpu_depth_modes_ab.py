"""k_features time of the depth path (limo_depth_last_kernel_ms): the default configuration on this tree's library against
another build of it (normally the parent commit's, scripts/build_baseline_lib.sh REV base) in ALTERNATING runs, a fresh
process per run, and the modes of the parameter file (tests/depth_modes_common.MODES with the file's own search window) on
this tree's library.  Full-size frames: seeds 1-3 at 2000 and 4000 azimuth steps, 1500 features; median of 30 launches.
    python scripts/gpu_depth_modes_ab.py [--rounds N] [--no-modes] [--out FILE.json] [--base LIB.so]
Stops at the first run that fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 30


def worker(modes):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import numpy as np

    import depth_modes_common as dm
    from limo_amd import ba, synth_lidar

    ctx = ba.Context(0)
    assert ctx.lib.limo_depth_set_timing(ctx.ptr, 1) == 0
    out = {"lib": os.environ.get("LIMO_HIP_LIB", "tree"), "modes": {}}
    frames = {}
    for s in (1, 2, 3):
        for az in (2000, 4000):
            fr = synth_lidar.make_frame(s)
            if az != 2000:
                fr["cloud"] = synth_lidar.make_sweep(s, n_az=az)
                fr["uv"], fr["is_ground"], fr["z_true"] = synth_lidar.make_features(fr["cloud"], s)
            frames[(s, az)] = fr
    for mode in modes:
        res = {}
        for (s, az), fr in frames.items():
            p = ba.depth_default_params()
            if mode != "default":
                p = dm.params_with({k: v for k, v in dm.MODES[mode].items() if k not in dm.WIDE}, p)  # the file's own window
            kf, tot = [], []
            for r in range(REPS + 3):
                d = ba.depth_estimate(ctx, fr, params=p)
                ms = ba.depth_kernel_ms(ctx)
                if r >= 3:
                    kf.append(ms["k_features"])
                    tot.append(ms["total"])
            res["seed%d_az%d" % (s, az)] = {"k_features_us_median": 1e3 * float(np.median(kf)), "k_features_us_min": 1e3 * float(np.min(kf)),
                                             "all_kernels_us_median": 1e3 * float(np.median(tot)), "accepted": int((d > 0).sum()), "n_feat": int(len(d))}
        out["modes"][mode] = res
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--no-modes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "depth_modes_ab.json"))
    ap.add_argument("--base", default=os.path.join(ROOT, "limo_amd", "lib", "variants", "liblimo_hip_base.so"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker.split(","))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    plan = [("base", "default"), ("tree", "default")] * a.rounds
    if not a.no_modes:
        plan.append(("tree", "radius,pca,clamp,corridor,triangle_patch,combined"))
    runs = []
    for tag, modes in plan:
        env = dict(os.environ)
        if tag == "base":
            env["LIMO_HIP_LIB"] = a.base
            env["LIMO_ALLOW_OLDER_ABI"] = "1"
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--worker", modes], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            print("FAILED", tag, modes, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
            return 1
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
        d["tag"] = tag
        runs.append(d)
        for mode, res in d["modes"].items():
            print(tag, mode, " ".join("%s %.2f" % (k, v["k_features_us_median"]) for k, v in res.items()), flush=True)
        json.dump(runs, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
