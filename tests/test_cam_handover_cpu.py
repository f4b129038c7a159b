"""What cam_assemble hands to cam_solve (limo_amd/csrc/kba_items.hpp): the scaled, undamped camera system of the free slots in the
solve's own enumeration, assembled from the block tridiagonal band of H_cc (cam_bt_index).  tests/cpp/test_cam_handover.cpp restates
the dense assembly - zero, add, mask, enumerate - and compares every entry of the hand-over with it as a 64-bit pattern, for seven
window shapes, with the Jacobi scale computed and kept; it also checks that cam_bt_index is a bijection of the band for 1..20
keyframes.  Stand-alone host program under -fsanitize=address,undefined with scratch vectors of exactly cam_assemble_scratch /
cam_solve_scratch doubles: an index that leaves the layout is caught."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_cam_handover_matches_dense_assembly_bit_for_bit():
    out = os.path.join(_HERE, "cpp", "_build", "test_cam_handover")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-std=c++17", "-pthread", "-o", out,
                           os.path.join(_HERE, "cpp", "test_cam_handover.cpp"), os.path.join(_HERE, "..", "limo_amd", "csrc", "kba_pack.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-6000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    # 60 bijection checks, and per window and pass one check per entry of the hand-over and per double behind it
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) >= 10000
