"""The per-window speed prior of a pose-only batch (limo_amd/csrc/kba_pack.hpp: PackOptions::per_window_prior / window_priors, what
limo_ba_batch_create_pose_only packs with) as a stand-alone host program (tests/cpp/test_pose_batch_pack.cpp), built under
-fsanitize=address together with kba_pack.cpp: every window of a batch is described as the same window packed alone, apart from its
offsets; NULL priors = all disabled; an invalid window fails the batch and is named by its index."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_pose_batch_pack_per_window_priors():
    out = os.path.join(_HERE, "cpp", "_build", "test_pose_batch_pack")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-ffp-contract=off", "-std=c++17", "-pthread", "-o", out,
                           os.path.join(_HERE, "cpp", "test_pose_batch_pack.cpp"), os.path.join(_HERE, "..", "limo_amd", "csrc", "kba_pack.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout and "AddressSanitizer" not in r.stderr
    # five windows of >= 12 landmarks with three checks per landmark alone are far more than this
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) >= 1000
