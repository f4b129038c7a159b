"""The class of ground-plane Schur groups (kba_layout.hpp:SchurGroup::gp_class, kba_items.hpp:schur_group_make with the row tables) and
the column map of the narrow tile, as a stand-alone host program (tests/cpp/test_schur_narrow.cpp) built under
-fsanitize=address,undefined: hand-made windows with all rows on the newest keyframe, rows on two keyframes inside one block and in
different blocks, rows only on a keyframe without a free plane slot, a last block of 6 landmarks, constant landmarks behind the
ground-plane run, the device route (no tables: always wide), the batch rule (two panels: nothing is classified); and for each class
that the map and its inverse cover exactly the slab entries slab_packed_read(true, ...) hands the camera solve, none twice.
Also: KBA_SCHUR_GP_WIDE is the last of the solve switches (tests/cpp/test_batch_plan.cpp builds and passes unchanged)."""
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def test_schur_narrow_classes_and_column_map():
    out = os.path.join(_HERE, "cpp", "_build", "test_schur_narrow")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-std=c++17", "-o", out, os.path.join(_HERE, "cpp", "test_schur_narrow.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) > 5000  # the maps are checked entry by entry


def test_switch_is_appended_and_read():
    src = open(os.path.join(_ROOT, "limo_amd", "csrc", "kba_batch_plan.hpp")).read()
    body = src[src.index("struct SolveSwitches {"):]
    body = body[: body.index("};")]
    fields = re.findall(r"^\s*(?:bool|int|double)\s+(\w+)", body, re.M)
    assert fields[-1] == "gp_wide", fields
    assert 's.gp_wide = on("KBA_SCHUR_GP_WIDE")' in src
