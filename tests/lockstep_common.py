"""Test infrastructure of the lock-step drive (limo_amd/kba/lockstep_driver.hpp, apps/limo_stream --sequences), shared by the CPU tier
(tests/test_lockstep_cpu.py), the GPU tier (tests/test_gpu_lockstep.py) and scripts/bench_lockstep.py: the stand-alone sanitized
builds of the app against the emulated C-ABI, the runner of a lock-step drive, and the single drives it is compared with (run once per
backend, frame count, seed and flags, shared by the tests that need them)."""
import json
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import emu_ffi  # noqa: E402

_BUILD = os.path.join(_HERE, "cpp", "_build")
_CSRC = os.path.join(_ROOT, "limo_amd", "csrc")
_KBA = os.path.join(_ROOT, "limo_amd", "kba")
APP_ASAN = os.path.join(_BUILD, "limo_stream_emu_asan")
APP_TSAN = os.path.join(_BUILD, "limo_stream_emu_tsan")
STAGES = ("depth", "five_point", "pose_only", "landmark_init", "select", "solve")
FIRST_CASE = ["--sequences", "3", "--frames", "24", "--frames-step", "4", "--stagger", "1", "--az", "2000", "--seed", "7"]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _sources():
    """The app, the shim and the emulated C-ABI with the oracle's depth assignment in ONE executable (the recipe of
    emu_ffi.build_stream_app(gpu=False), without the shared library in between: the sanitizer sees every frame of it)."""
    return [emu_ffi.STREAM_APP_SRC] + emu_ffi.SHIM_SRC + emu_ffi._SRC + [os.path.join(_CSRC, "host_misc.cpp")]


def _deps():
    deps = _sources() + [os.path.join(_ROOT, "include", "limo_hip.h"), os.path.join(_ROOT, "apps", "limo_stream", "synth_world.hpp")]
    for d in (_CSRC, _KBA):
        deps += [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".hpp")]
    return deps


def _compile(out, sanitize):
    oracle_dir = os.path.abspath(os.path.join(_ROOT, "oracle", "_build"))
    if not os.path.exists(os.path.join(oracle_dir, "liboracle.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(_ROOT, "oracle")])
    cmd = ["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-std=c++17", "-pthread", "-DKBA_EMU_EXPORT_ABI", "-DKBA_EMU_DEPTH"] + sanitize
    return subprocess.run(cmd + ["-o", out] + _sources() + ["-L" + oracle_dir, "-loracle", "-Wl,-rpath," + oracle_dir], capture_output=True, text=True)


def build_asan():
    """limo_stream on the emulator under -fsanitize=address,undefined: a host program with its own main."""
    os.makedirs(_BUILD, exist_ok=True)
    if _stale(APP_ASAN, _deps()):
        r = _compile(APP_ASAN, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
        if r.returncode != 0:
            raise RuntimeError("limo_stream_emu_asan does not compile:\n" + r.stderr[-4000:])
    return APP_ASAN


def build_tsan():
    """The same under -fsanitize=thread.  None where the toolchain has no ThreadSanitizer runtime (the link fails on -ltsan)."""
    os.makedirs(_BUILD, exist_ok=True)
    if _stale(APP_TSAN, _deps()):
        r = _compile(APP_TSAN, ["-fsanitize=thread"])
        if r.returncode != 0:
            if "tsan" in r.stderr and ("cannot find" in r.stderr or "No such file" in r.stderr):
                return None
            raise RuntimeError("limo_stream_emu_tsan does not compile:\n" + r.stderr[-4000:])
    return APP_TSAN


def build():
    build_asan()
    build_tsan()


def run_lockstep(exe, args, poses, timeout=600, env=None):
    """One lock-step drive: (the JSON line as a dict, [bytes of poses.0, poses.1, ...])."""
    r = subprocess.run([exe] + list(args) + ["--quiet", "--poses", poses], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    info = json.loads(r.stdout.strip().splitlines()[-1])
    files = [open("%s.%d" % (poses, i), "rb").read() for i in range(info["sequences"])]
    return info, files


_single = {}


def single_rows(exe, frames, seed, extra, tmp_dir, timeout=600):
    """The pose file of the single drive (StreamDriver) of `frames` frames and `seed`; run once per distinct drive."""
    key = (exe, frames, seed, tuple(extra))
    if key not in _single:
        path = os.path.join(str(tmp_dir), "single_%d_%d_%d.txt" % (frames, seed, len(_single)))
        r = subprocess.run([exe, "--frames", str(frames), "--seed", str(seed), "--quiet", "--poses", path] + list(extra), capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        info = {l.split()[0]: float(l.split()[1]) for l in r.stdout.splitlines() if len(l.split()) == 2 and l.split()[0] in ("frames", "keyframes", "solves")}
        _single[key] = (open(path, "rb").read(), info)
    return _single[key]
