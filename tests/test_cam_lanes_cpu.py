"""The 128-lane form of the camera kernels (limo_amd/csrc/kba_items.hpp: cam_assemble / cam_solve with 128 lanes that stand in for 256
virtual ones) must leave the bits of the 256-lane form.  tests/cpp/test_cam_lanes.cpp runs the host statements of both functions as a
workgroup runs them - the lanes are threads that meet at KBA_SYNC - with 128 and with 256 lanes on windows of 2 and of 5 keyframes,
with the Jacobi scale computed and kept, and compares the hand-over region, g_c, the scale, the regulariser costs, WinRed, the camera
step and the candidate poses as 64-bit patterns; one lane alone must differ somewhere (the comparison can tell).  Stand-alone host
program under -fsanitize=address,undefined with scratch vectors of exactly the layouts' sizes."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_cam_lanes_128_leave_the_bits_of_256():
    out = os.path.join(_HERE, "cpp", "_build", "test_cam_lanes")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-std=c++17", "-pthread", "-o", out, os.path.join(_HERE, "cpp", "test_cam_lanes.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-6000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    # per window and pass one check per double the two launches leave (hand-over, g_c, scale, reductions, step, candidates, view constants)
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) >= 10000
