"""The problem's rules of the pack (limo_amd/csrc/kba_pack.hpp: build_window_problem - which residual and parameter blocks a window
has, in the caller's indices) as a stand-alone host program (tests/cpp/test_window_problem.cpp), built under
-fsanitize=address,undefined together with kba_pack.cpp: ground-plane rows, scale and ground-plane regularisers, present / free camera
slots, landmark states, view order, trimming flag and the pose-only prior, each against values written out from the rule; and the
option pair pack_windows refuses (evaluate-only with landmark shards)."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_window_problem_rules():
    out = os.path.join(_HERE, "cpp", "_build", "test_window_problem")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (-O0: under both sanitizers an optimised build of kba_pack.cpp takes a minute to compile, this one seconds)
    subprocess.check_call(["g++", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-std=c++17", "-pthread",
                           "-o", out, os.path.join(_HERE, "cpp", "test_window_problem.cpp"), os.path.join(_HERE, "..", "limo_amd", "csrc", "kba_pack.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    # every group of cases ran (the file has 133 checks; the slot cases alone are 36 of them)
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) >= 120
