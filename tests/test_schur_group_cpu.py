"""The Schur group record (kba_layout.hpp:SchurGroup, written at pack time by kba_items.hpp:schur_group_make and read by every lean Schur
wave before its first load) against values written out from the window's layout, as a stand-alone host program
(tests/cpp/test_schur_group.cpp) built under -fsanitize=address: both span pairs, both classes, a clipped last group, a free keyframe
without a view, idle keyframe entries, slab offsets in both layouts."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_schur_group_record():
    out = os.path.join(_HERE, "cpp", "_build", "test_schur_group")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-ffp-contract=off", "-std=c++17", "-o", out,
                           os.path.join(_HERE, "cpp", "test_schur_group.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout and "AddressSanitizer" not in r.stderr
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) == 45  # seven groups of six checks, two on idle entries, one on the size
