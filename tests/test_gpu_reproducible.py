"""Every device entry point returns the same bits when it is called again with the same input, also when other calls
of different sizes run in between (pooled blocks get reused), and the results do not depend on what a device block
held before (KBA_POISON=1 fills every block with NaN bytes at allocation)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from limo_amd import ba, default_options, synth, synth_lidar
from test_emu_vs_oracle import make_pose_only_case
from test_gpu_landmark_init import _rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _solve_infos(stdout):
    """The 'solve info' lines of scripts/gpu_poison_check.py (one per case, next to its checksum line) as dicts."""
    out = []
    for l in stdout.splitlines():
        if " solve info " in l:
            d = dict(kv.split("=") for kv in l.split(" solve info ")[1].split())
            out.append({k: (v if k == "path" else int(v)) for k, v in d.items()})
    return out


def test_repeated_calls_give_the_same_bits(ctx):
    o = default_options()
    rng = np.random.default_rng(5)
    off, rays, use_depth, _ = _rays(rng, 2000)
    pw, prior, _ = make_pose_only_case(71)
    po = default_options(min_landmarks_for_trimming=30)
    fr = synth_lidar.make_frame(1)
    ref = {}
    for rep in range(6):
        pos, ok = ctx.landmark_init(off, rays, use_depth)
        w = synth.make_window(7001, n_lm=600)
        r = ctx.solve(w, o)
        p = pw.copy()
        rp = ctx.adjust_pose_only(p, prior, po)
        d = np.asarray(ba.depth_estimate(ctx, fr))
        ctx.solve(synth.make_window(9000 + rep, n_lm=150 + 40 * rep), o)  # something of another size in between
        got = {
            "landmark_init": (pos[ok.astype(bool)].tobytes(), ok.tobytes()),
            "solve": (w.kf_pose.tobytes(), w.lm_pos.tobytes(), r["final_cost"], r["iterations_total"]),
            "pose_only": (p.kf_pose.tobytes(), rp["final_cost"], rp["iterations_total"]),
            "depth": d.tobytes(),
        }
        if not ref:
            ref = got
        for k in got:
            assert got[k] == ref[k], "%s differs on repetition %d" % (k, rep)


def test_results_do_not_depend_on_stale_device_memory():
    out = []
    for poison in (False, True):
        env = dict(os.environ)
        env.pop("KBA_POISON", None)
        if poison:
            env["KBA_POISON"] = "1"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gpu_poison_check.py")], capture_output=True, text=True, timeout=600,
                           env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if "checksum" in l]
        assert len(lines) == 6
        out.append(lines)
    assert out[0] == out[1]
    assert all(" nan 0 " in l and " unchanged 0 " in l for l in out[0])


def test_linearisation_variants_give_the_same_bits():
    """k_lin_lm exists twice: <true> (default: view constants, landmark sums and tail inputs in LDS) and <false> (KBA_LIN_VLDS=0:
    scalar loads of the view constants - also what batches with many views per window take).  The same statements in the same order:
    every checksum of the poison script must be the same to the last bit whichever one runs."""
    out = []
    for extra, variant in (({}, 1), ({"KBA_LIN_VLDS": "0"}, 0)):
        env = dict(os.environ, **extra)
        env.pop("KBA_POISON", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gpu_poison_check.py"), "short"], capture_output=True, text=True, timeout=600,
                           env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if "checksum" in l]
        assert len(lines) >= 3
        out.append(lines)
        # k_lin_lm is launched by the launch sequences; the one-launch kernels contain the LDS form whatever the switch says
        infos = _solve_infos(r.stdout)
        assert len(infos) == len(lines)
        launched = [i for i in infos if i["path"] in ("STREAMING", "LOCKSTEP")]
        assert launched and all(i["lin_variant"] == variant for i in launched), infos
        assert all(i["lin_variant"] == 1 for i in infos if i["path"] in ("WG", "COOP")), infos
    assert out[0] == out[1]


def test_schur_pair_launch_gives_the_same_bits():
    """The draining rounds of the streaming solve take both fast-class Schur lists in one launch (k_schur_lean_pair);
    KBA_NO_SCHUR_PAIR=1 launches the two lists separately - the same device functions on the same slabs: the same bits."""
    out = []
    for extra in ({}, {"KBA_NO_SCHUR_PAIR": "1"}):
        env = dict(os.environ, **extra)
        env.pop("KBA_POISON", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gpu_poison_check.py")], capture_output=True, text=True, timeout=900,
                           env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if "checksum" in l]
        assert len(lines) == 6
        out.append(lines)
        infos = _solve_infos(r.stdout)
        assert len(infos) == 6
        pairs = sum(i["pair_launches"] for i in infos if i["path"] == "STREAMING")
        assert sum(i["pair_launches"] for i in infos) == pairs  # (only the streaming solve launches the pair kernel)
        assert (pairs == 0) if extra else (pairs > 0), infos
    assert out[0] == out[1]
