#!/usr/bin/env python3
"""Lock-step drive against single drives: aggregate frames/s of `limo_stream --sequences N` for N in 1, 4, 16, 64 with the default
stage flags and with every stage on the device (--select-device --five-point-prior --five-point-device), against N single drives of
the PARENT commit's limo_stream run one after another (the only way to run N sequences before the lock-step driver); and the single
drive of this commit against the parent's, runs alternated, to show what the split-phase shim costs the single driver.

  scripts/bench_lockstep.py --build-parent REV      (on the build machine: needs git) compiles REV's apps/limo_stream + shim against the
                                                    liblimo_hip.so of the work tree into tests/cpp/_build/limo_stream_gpu_parent
  scripts/bench_lockstep.py [--frames 200] [--sizes 1,4,16,64] [--repeats 3] [--out profiles/lockstep.json]   (on the GPU machine)
  scripts/bench_lockstep.py --against-parent [--frames 200] [--repeats 3] [--out ...]   (on the GPU machine) for a change of the drivers'
                                                    host side when REV already has the lock-step driver: the parent's `--sequences N` too,
                                                    alternated with this commit's, and the single drives with both flag sets
  scripts/bench_lockstep.py --sweep 16 [--frames 200] [--out ...]   (on the GPU machine) a sweep of 16 parameter sets - depth_thres x
                                                    reprojection_thres, 4 x 4 of the reference's tune_parameters_kitti.py grid - over ONE world in
                                                    lock step (`--sequences 16 --sweep FILE`: the file is written here), against the same 16
                                                    drives of this commit's limo_stream run one after another with the parameters as flags

The kernels are the same in both programs (this comparison is only fair while limo_amd/csrc is unchanged between REV and the work
tree: --build-parent refuses otherwise).  Every process runs under its own time limit; a failing run ends the script.  The table goes to
stdout, everything measured to --out as JSON."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(BUILD, "limo_stream_gpu")
PARENT = os.path.join(BUILD, "limo_stream_gpu_parent")
DEVICE_FLAGS = ["--select-device", "--five-point-prior", "--five-point-device"]
STAGES = ("depth", "five_point", "pose_only", "landmark_init", "select", "solve")


def build_parent(rev):
    changed = subprocess.run(["git", "diff", "--stat", rev, "--", "limo_amd/csrc", "include/limo_hip.h"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    if changed:
        sys.exit("the kernels differ between %s and the work tree: the two programs would not run the same library\n%s" % (rev, changed))
    tmp = tempfile.mkdtemp(prefix="limo_parent.")
    try:
        tar = subprocess.Popen(["git", "archive", rev, "apps", "limo_amd/kba", "limo_amd/csrc", "include"], cwd=ROOT, stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", tmp], stdin=tar.stdout)
        assert tar.wait() == 0
        libdir = os.path.join(ROOT, "limo_amd", "lib")
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-w", "-o", PARENT, os.path.join(tmp, "apps", "limo_stream", "limo_stream.cpp"),
                               os.path.join(tmp, "limo_amd", "kba", "bundle_adjuster_keyframes.cpp"), "-L" + libdir, "-llimo_hip", "-Wl,-rpath," + os.path.abspath(libdir)])
    finally:
        shutil.rmtree(tmp)
    open(PARENT + ".rev", "w").write(subprocess.run(["git", "rev-parse", rev], cwd=ROOT, capture_output=True, text=True, check=True).stdout)
    print(PARENT)


def run(cmd, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("%s\nexit %d\n%s\n%s" % (" ".join(cmd), r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return r.stdout, wall


def single(exe, frames, seed, flags, limit):
    """One single drive: (fps of the pipeline as the program reports it, seconds of pipeline time, wall seconds of the process)."""
    out, wall = run([exe, "--frames", str(frames), "--az", "2000", "--seed", str(seed), "--quiet"] + flags, limit)
    kv = {l.split()[0]: float(l.split()[1]) for l in out.splitlines() if len(l.split()) == 2 and l.split()[0] in ("frames", "fps")}
    return kv["fps"], kv["frames"] / kv["fps"], wall


def lockstep(exe, n, frames, flags, limit):
    out, wall = run([exe, "--sequences", str(n), "--frames", str(frames), "--az", "2000", "--seed", "7", "--quiet"] + flags, limit)
    info = json.loads(out.strip().splitlines()[-1])
    info["wall_s"] = wall
    del info["per_sequence"]
    return info


def sweep_lines(n):
    """n parameter sets: the corner of tune_parameters_kitti.py's grid (10 x 11 values of robust_loss_depth_thres x
    robust_loss_reprojection_thres) this many sequences cover, row by row."""
    depth = [0.04 * (i + 1) for i in range(10)]
    repro = [0.4 * (i + 1) for i in range(11)]
    side = max(1, int(round(n ** 0.5)))
    return [(depth[(k // side) % 10], repro[(k % side) % 11]) for k in range(n)]


def sweep(a):
    """`--sequences N --sweep FILE` against the N single drives with flags, one after another: frames/s of both, the share of
    batched bundle-adjustment calls that carried differing options, and the sweep's own result (parameters -> ATE)."""
    if not os.path.exists(EXE):
        sys.exit("%s is missing (build())" % EXE)
    n = a.sweep
    sets = sweep_lines(n)
    with tempfile.NamedTemporaryFile("w", suffix=".sweep", delete=False) as f:
        for d, r in sets:
            f.write("depth_thres=%r reprojection_thres=%r\n" % (d, r))
        path = f.name
    try:
        out, wall = run([EXE, "--sequences", str(n), "--frames", str(a.frames), "--az", "2000", "--seed", "7", "--quiet", "--sweep", path], a.limit)
    finally:
        os.unlink(path)
    info = json.loads(out.strip().splitlines()[-1])
    info["wall_s"] = wall
    secs = [single(EXE, a.frames, 7, ["--depth-thres", repr(d), "--reprojection-thres", repr(r)], a.limit)[1] for d, r in sets]
    base = n * a.frames / sum(secs)
    st = info["stages"]
    print("sweep of %d parameter sets, %d frames each: lock step %.1f frames/s (%.2f ms per tick) | %d single drives one after another %.1f frames/s | x %.2f" % (
        n, a.frames, info["frames_per_s"], info["ms_pipeline"] / max(1, info["ticks"]), n, base, info["frames_per_s"] / base))
    for name in ("pose_only", "solve"):
        print("  %-9s %d batched calls (%d with an entry of options per window), most items %d, %d single-call fallbacks, %.2f ms per tick inside the C-ABI" % (
            name, st[name]["batched_calls"], st[name]["per_window_calls"], st[name]["max_items"], st[name]["fallback_calls"], st[name]["ms_abi"] / max(1, info["ticks"])))
    print("  depth_thres reprojection_thres  ATE rmse [m]")
    for p in info["per_sequence"]:
        print("  %11.2f %18.1f  %.4f" % (p["depth_thres"], p["reprojection_thres"], p["ate_rmse"]))
    res = {"frames": a.frames, "sets": n, "lockstep": info, "single_pipeline_s": secs, "single_frames_per_s": base, "speedup": info["frames_per_s"] / base}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


def against_parent(a):
    """Host-side changes of the drivers, this commit against a parent that HAS the lock-step driver: per row the parent, the parent
    again and this commit, alternated, a.repeats runs each.  The two parent series are the same program: all their runs together give
    the box's spread (half their range over their median), and this commit's median has to lie within it of the parent's."""
    rows = [("single, default flags", lambda exe: single(exe, a.frames, 7, [], a.limit)[0]),
            ("single, every stage on the device", lambda exe: single(exe, a.frames, 7, DEVICE_FLAGS, a.limit)[0])]
    rows += [("lock step, N = %d, default flags" % n, lambda exe, n=n: lockstep(exe, n, a.frames, [], a.limit)) for n in (1, 16)]
    res = {"frames": a.frames, "parent_rev": open(PARENT + ".rev").read().strip() if os.path.exists(PARENT + ".rev") else None, "rows": []}
    for name, drive in rows:
        runs = {"parent": [], "parent_again": [], "this": []}
        for _ in range(a.repeats):
            for series, exe in (("parent", PARENT), ("parent_again", PARENT), ("this", EXE)):
                runs[series].append(drive(exe))
        fps = {k: [r["frames_per_s"] if isinstance(r, dict) else r for r in v] for k, v in runs.items()}
        both = fps["parent"] + fps["parent_again"]
        parent = statistics.median(both)
        spread = (max(both) - min(both)) / 2 / parent
        delta = statistics.median(fps["this"]) / parent - 1
        row = {"row": name, "frames_per_s": fps, "median_parent": parent, "median_this": statistics.median(fps["this"]), "spread": spread, "delta": delta, "within_spread": abs(delta) <= spread}
        if isinstance(runs["this"][0], dict):  # where the host time of a tick goes, per stage: median of the runs, ms per tick
            row["ms_host_per_tick"] = {k: {s: statistics.median(r["stages"][s]["ms_host"] / max(1, r["ticks"]) for r in runs[k]) for s in STAGES} for k in runs}
        res["rows"].append(row)
        print("%-36s parent %s | again %s | this %s | medians %.1f -> %.1f (%+.1f %%), spread of the parent +-%.1f %%: %s" % (
            name, " ".join("%.1f" % x for x in fps["parent"]), " ".join("%.1f" % x for x in fps["parent_again"]), " ".join("%.1f" % x for x in fps["this"]), parent,
            row["median_this"], 100 * delta, 100 * spread, "within" if row["within_spread"] else "OUTSIDE"))
        sys.stdout.flush()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-parent", metavar="REV")
    ap.add_argument("--against-parent", action="store_true", help="the single and the lock-step drive (N = 1, 16) of this commit against the parent's, alternated, with the box's spread")
    ap.add_argument("--sweep", type=int, metavar="N", help="N parameter sets over one world in lock step against the N single drives with flags, one after another")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--sizes", default="1,4,16,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-drives", type=int, default=4, help="single drives of the parent timed per flag set (seeds 7, 8, ...): N drives one after another take N x their mean")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep.json"))
    a = ap.parse_args()
    if a.build_parent:
        return build_parent(a.build_parent)
    if a.sweep:
        return sweep(a)
    for exe in (EXE, PARENT):
        if not os.path.exists(exe):
            sys.exit("%s is missing (build(); scripts/bench_lockstep.py --build-parent REV)" % exe)
    if a.against_parent:
        return against_parent(a)
    res = {"frames": a.frames, "parent_rev": open(PARENT + ".rev").read().strip() if os.path.exists(PARENT + ".rev") else None, "single": {}, "baseline": {}, "lockstep": []}
    # 1. the single drive: this commit against the parent, alternated
    runs = {"parent": [], "this": []}
    for _ in range(a.repeats):
        for name, exe in (("parent", PARENT), ("this", EXE)):
            runs[name].append(single(exe, a.frames, 7, [], a.limit)[0])
    res["single"] = {k: {"fps": v, "median": statistics.median(v)} for k, v in runs.items()}
    print("single drive, %d frames, frames/s (alternated): parent %s | this commit %s" % (a.frames, " ".join("%.1f" % x for x in runs["parent"]), " ".join("%.1f" % x for x in runs["this"])))
    # 2. the baseline: single drives of the parent, one after another (seconds of pipeline time per drive; N drives take N x that)
    for name, flags in (("default", []), ("device", DEVICE_FLAGS)):
        secs = [single(PARENT, a.frames, 7 + i, flags, a.limit)[1] for i in range(a.baseline_drives)]
        res["baseline"][name] = {"pipeline_s_per_drive": secs, "frames_per_s": a.frames / statistics.mean(secs)}
        print("baseline (%s flags): %d single drives of the parent one after another: %.1f frames/s" % (name, len(secs), res["baseline"][name]["frames_per_s"]))
    # 3. the lock-step drive
    print("%-8s %4s %10s %9s %9s | per tick, ms: %s | host finish" % ("flags", "N", "frames/s", "x base", "ms/tick", " ".join("%-13s" % s for s in STAGES)))
    for name, flags in (("default", []), ("device", DEVICE_FLAGS)):
        for n in [int(x) for x in a.sizes.split(",")]:
            info = lockstep(EXE, n, a.frames, flags, a.limit)
            info["flags"] = name
            info["speedup_over_baseline"] = info["frames_per_s"] / res["baseline"][name]["frames_per_s"]
            res["lockstep"].append(info)
            ticks = max(1, info["ticks"])
            per = " ".join("%5.2f+%-7.2f" % (info["stages"][s]["ms_host"] / ticks, info["stages"][s]["ms_abi"] / ticks) for s in STAGES)
            print("%-8s %4d %10.1f %9.2f %9.2f | host+abi: %s | %.2f" % (name, n, info["frames_per_s"], info["speedup_over_baseline"], info["ms_pipeline"] / ticks, per,
                                                                    info["ms_host_finish"] / ticks))
            sys.stdout.flush()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
