"""The per-batch kernel plan, the Schur worklist builder and the plan of one solve (limo_amd/csrc/kba_batch_plan.hpp: which k_schur_lean /
k_schur_wide variant a batch gets, the LDS sizes, the order of a worklist; which launch path a solve takes under every KBA_* switch, the
cooperative grid, the slot groups of a streaming solve) and the pack arena's lend guard (kba_pack.hpp:PackArenaLend) as a stand-alone host
program (tests/cpp/test_batch_plan.cpp), built under -fsanitize=address together with kba_pack.cpp."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_batch_plan_worklists_and_lend_guard():
    out = os.path.join(_HERE, "cpp", "_build", "test_batch_plan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-ffp-contract=off", "-std=c++17", "-pthread", "-o", out,
                           os.path.join(_HERE, "cpp", "test_batch_plan.cpp"), os.path.join(_HERE, "..", "limo_amd", "csrc", "kba_pack.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) >= 69 + 100  # six fast-class rows of 7 checks and nine generic ones of 3 alone are 69; the solve plan adds > 100
