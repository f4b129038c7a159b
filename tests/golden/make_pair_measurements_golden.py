"""Generates tests/golden/pair_measurements_emu.json: what the emulated pipeline computes on the shapes of tests/pair_meas_common.py
(pair_meas_common.record: report counts, costs and keyframe parameters as hex floats, landmark digests, trimmed landmarks).

The committed file holds the bits of the emulator as it was BEFORE the pair-indexed measurement planes (commit 51087aa): --rev builds
that commit's emulator (its limo_amd/csrc and tests/cpp, `git archive` into a scratch directory, the flags of tests/fixed_lm_common.py)
and records what IT computes; tests/test_pair_measurements_cpu.py holds today's emulator to those bits.  Without --rev the file is
written from today's emulator (only right after a change that is MEANT to move bits).

Run from the repo root:  python tests/golden/make_pair_measurements_golden.py [--rev 51087aa]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tarfile
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import fixed_lm_common as flc  # noqa: E402
import pair_meas_common as pmc  # noqa: E402
from limo_amd import default_options  # noqa: E402


def emulator_of(rev, tmp):
    """libkba_emu_fixed.so built from the sources of `rev`."""
    tar = os.path.join(tmp, "src.tar")
    subprocess.check_call(["git", "-C", ROOT, "archive", "-o", tar, rev, "limo_amd/csrc", "tests/cpp", "include"])
    with tarfile.open(tar) as t:
        t.extractall(tmp)
    lib = os.path.join(tmp, "libkba_emu_fixed.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-fPIC", "-shared", "-o", lib,
                           os.path.join(tmp, "tests", "cpp", "emu_fixed_lm.cpp"), os.path.join(tmp, "limo_amd", "csrc", "kba_pack.cpp")])
    return lib


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        source = "this tree"
        if "--rev" in sys.argv:
            rev = sys.argv[sys.argv.index("--rev") + 1]
            today = flc.emu()  # (binds the argument types; the entries of the other build take the same)
            lib = C.CDLL(emulator_of(rev, tmp))
            for fn in ("emu_ba_solve_batch_fixed", "emu_last_trimmed"):
                getattr(lib, fn).argtypes = getattr(today, fn).argtypes
            flc._emu = lib
            source = "the emulator of commit " + rev
        gold = {"generator": "tests/golden/make_pair_measurements_golden.py", "emulator": source, "cases": pmc.solve_all(default_options())}
    with open(os.path.join(HERE, "pair_measurements_emu.json"), "w") as f:
        json.dump(gold, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d cases from %s" % (len(gold["cases"]), source))
