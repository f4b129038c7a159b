"""Who takes which form of the camera kernels (limo_amd/csrc/kba_batch_plan.hpp): per batch (plan_cam_lanes: LDS-class windows of at most
128 slots, an unsharded solve batch, at least twice the workgroups per CU), per launch (cam_lanes_for_launch: more windows listed than
the 256-lane form holds resident) and the KBA_CAM_LANES switch of read_solve_switches, as a stand-alone host program
(tests/cpp/test_cam_lanes_plan.cpp) under -fsanitize=address,undefined together with kba_pack.cpp."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_cam_lanes_plan_rule_and_switch():
    out = os.path.join(_HERE, "cpp", "_build", "test_cam_lanes_plan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-std=c++17", "-pthread", "-o", out,
                           os.path.join(_HERE, "cpp", "test_cam_lanes_plan.cpp"), os.path.join(_HERE, "..", "limo_amd", "csrc", "kba_pack.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) >= 35  # 13 on the batch rule, 11 on the launch rule, the rest on the switch
