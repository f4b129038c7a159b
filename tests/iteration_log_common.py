"""Test infrastructure of the per-iteration solver log (include/limo_hip.h:limo_ba_iteration), shared by the CPU tier
(tests/test_iteration_log_cpu.py) and the GPU tier (tests/test_gpu_iteration_log.py): the four test windows, the emulator entry
that records the log (tests/cpp/emu_iteration_log.cpp), the oracle's table (ORACLE_VERBOSE=1 in a child process without the GPU) and
the checks both tiers apply to a log - the identities every log satisfies, and the comparison with the oracle's table.

Run as a script (`python iteration_log_common.py oracle NAME`) it is that child process."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), _HERE):  # (as tests/conftest.py: the child process has no conftest)
    if _p not in sys.path:
        sys.path.insert(0, _p)

from limo_amd import _ffi, default_options, synth  # noqa: E402
from limo_amd.window import struct_array  # noqa: E402

_BUILD = os.path.join(_HERE, "cpp", "_build")
_CSRC = os.path.join(_ROOT, "limo_amd", "csrc")
EMU_LIB = os.path.join(_BUILD, "libkba_emu_itlog.so")
UNIT = os.path.join(_BUILD, "test_iteration_log")
UNIT_SAN = os.path.join(_BUILD, "test_iteration_log_san")
TOL = 1e-4  # the project's parity bar (tests/test_gpu_ba.py)
DTYPE = _ffi.iteration_dtype()
_emu = None


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _headers():
    return [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")] + [os.path.join(_ROOT, "include", "limo_hip.h")]


def build_unit():
    """tests/cpp/test_iteration_log.cpp, plain and under -fsanitize=address,undefined (a stand-alone host program)."""
    os.makedirs(_BUILD, exist_ok=True)
    src = os.path.join(_HERE, "cpp", "test_iteration_log.cpp")
    if _stale(UNIT, [src] + _headers()):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-o", UNIT, src])
    if _stale(UNIT_SAN, [src] + _headers()):
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                               "-ffp-contract=off", "-std=c++17", "-o", UNIT_SAN, src])
    return UNIT, UNIT_SAN


def build():
    os.makedirs(_BUILD, exist_ok=True)
    emu_src = [os.path.join(_HERE, "cpp", "emu_iteration_log.cpp"), os.path.join(_CSRC, "kba_pack.cpp")]
    if _stale(EMU_LIB, emu_src + [os.path.join(_HERE, "cpp", "emu_pipeline.cpp")] + _headers()):  # (tests/emu_ffi.py's flags)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-fPIC", "-shared", "-o", EMU_LIB] + emu_src)
    build_unit()


def emu():
    global _emu
    if _emu is None:
        build()
        _emu = C.CDLL(EMU_LIB)
        _emu.emu_ba_solve_batch_log.argtypes = [C.c_int32, C.POINTER(_ffi.BaWindow), C.POINTER(_ffi.c_uint8_p), C.POINTER(_ffi.BaOptions),
                                                C.POINTER(_ffi.BaReport), C.c_int, C.POINTER(_ffi.SpeedPrior), C.c_int, C.c_int32,
                                                C.POINTER(_ffi.BaIteration), _ffi.c_int32_p]
    return _emu


# ------------------------------------------------------------------------------------------------ the windows
NAMES = ("A", "B", "C", "P")
ORACLE_NAMES = ("B", "C", "P")  # A's iteration count moves under 1-ulp input changes: consistency and path identity only


def options(name):
    o = default_options()
    if name == "P":
        o.min_landmarks_for_trimming = 30
    return o


def window(name):
    """(window, prior or None) of a test window - the smallest shapes that still carry each feature of the schedule."""
    if name == "A":
        return synth.make_window(300, n_kf=3, n_lm=60), None
    if name == "B":
        return synth.make_window(301, n_kf=3, n_lm=150), None
    if name == "C":
        return synth.make_window(302, n_kf=4, n_lm=400, ground_frac=0.2), None
    if name == "P":
        w, prior, _ = synth.make_pose_only_case(71)
        return w, prior
    raise KeyError(name)


def schedule_bound(o):
    """Entries a window can record at most: the exact bound of the schedule (limo_hip.h)."""
    t = o.trim_solver_iterations
    return o.num_trim_rounds * ((t + 1) + (3 * t + 1)) + (o.max_num_iterations + 1)


def emu_solve(windows, opts, pose_only=False, prior=None, n_slots=0, lm_fixed=None):
    """The emulated pipeline on `windows` IN PLACE, lock-step (n_slots = 0) or streaming.  Returns (reports, logs)."""
    lib = emu()
    arr = struct_array(windows)
    n = len(windows)
    reps = (_ffi.BaReport * n)()
    cap = schedule_bound(opts)
    log = np.zeros((n, cap), DTYPE)
    log_n = np.zeros(n, np.int32)
    ptrs = None
    if lm_fixed is not None:
        keep = [None if f is None else np.ascontiguousarray(f, np.uint8) for f in lm_fixed]
        ptrs = (_ffi.c_uint8_p * n)(*[None if f is None else f.ctypes.data_as(_ffi.c_uint8_p) for f in keep])
    rc = lib.emu_ba_solve_batch_log(n, arr, ptrs, C.byref(opts), reps, int(pose_only), None if prior is None else C.byref(prior), int(n_slots), cap,
                                    log.ctypes.data_as(C.POINTER(_ffi.BaIteration)), log_n.ctypes.data_as(_ffi.c_int32_p))
    if rc != 0:
        raise RuntimeError("emu_ba_solve_batch_log rc=%d" % rc)
    assert (log_n <= cap).all()
    return [r.as_dict() for r in reps], [log[i, : log_n[i]].copy() for i in range(n)]


# ------------------------------------------------------------------------------------------------ the oracle's table
_ROW = re.compile(r"^\s+it\s+(\d+) cost (\S+) change (\S+) \|g\| (\S+) step (\S+) rho (\S+) radius (\S+) valid (\d) succ (\d)\s*$")


def parse_table(text):
    """ORACLE_VERBOSE output (oracle/kba_oracle.cpp:print_summary) -> list of solves, each a list of row dicts."""
    solves = []
    for line in text.splitlines():
        if line.startswith("solve:"):
            solves.append([])
            continue
        m = _ROW.match(line)
        if m:
            g = m.groups()
            solves[-1].append({"iteration": int(g[0]), "cost": float(g[1]), "cost_change": float(g[2]), "gradient_max_norm": float(g[3]),
                               "step_norm": float(g[4]), "relative_decrease": float(g[5]), "trust_region_radius": float(g[6]),
                               "radius_text": g[6], "step_is_valid": int(g[7]), "step_is_successful": int(g[8])})
    return solves


@functools.lru_cache(maxsize=None)
def oracle_table(name):
    """(solves, report) of the oracle on a test window: a child process with ORACLE_VERBOSE=1 whose stdout is parsed (the child
    never opens the GPU).  Computed once per process and shared."""
    env = dict(os.environ, ORACLE_VERBOSE="1", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "oracle", name], env=env, stdout=subprocess.PIPE, check=True, text=True).stdout
    rep = None
    for line in out.splitlines():
        if line.startswith("REPORT "):
            rep = json.loads(line[len("REPORT "):])
    assert rep is not None, out
    return parse_table(out), rep


def _oracle_child(name):
    import pyoracle

    w, prior = window(name)
    o = options(name)
    rep = pyoracle.adjust_pose_only(w, prior, o) if name == "P" else pyoracle.solve(w, o)[0]
    sys.stdout.flush()
    print("REPORT " + json.dumps(rep), flush=True)


def oracle_iterations_stable(name, n=8):
    """The oracle's own iteration count under n one-ulp changes of the input (fuzz_common.input_sensitivity): (min, max)."""
    import fuzz_common as fc
    import pyoracle

    w, prior = window(name)
    if name == "P":
        # (input_sensitivity solves with the default options; the pose-only window's trimming threshold goes in through the closure)
        def solve_o(x, _o):
            return pyoracle.adjust_pose_only(x, prior, options(name))
    else:
        def solve_o(x, o):
            return pyoracle.solve(x, o)[0]
    return fc.input_sensitivity(w, solve_o, n=n)["iterations"]


# ------------------------------------------------------------------------------------------------ checks
def _bits(x):
    return np.float64(x).view(np.uint64)


def split_solves(log):
    """The entries per `solve` value, in order."""
    out = []
    for e in log:
        if not out or out[-1][-1]["solve"] != e["solve"]:
            out.append([])
        out[-1].append(e)
    return out


def check_consistency(log, rep, o, where=""):
    """The identities every log satisfies - exact unless stated.  Returns {"rejected": n, "invalid": n} of the log."""
    assert log.dtype == DTYPE and log.dtype.itemsize == 64
    assert len(log) <= schedule_bound(o), where
    solves = split_solves(log)
    assert [s[0]["solve"] for s in solves] == list(range(len(solves))), where
    assert len(solves) == rep["num_solves"], (where, len(solves), rep["num_solves"])
    assert (log["pad"] == 0).all()
    n_rej = n_inv = 0
    for si, s in enumerate(solves):
        assert [int(e["iteration"]) for e in s] == list(range(len(s))), (where, si)
        assert len({int(e["solve_kind"]) for e in s}) == 1 and int(s[0]["solve_kind"]) in (0, 1, 2), (where, si)
        e0 = s[0]
        assert e0["cost_change"] == 0.0 and e0["step_norm"] == 0.0 and e0["relative_decrease"] == 0.0, (where, si)
        assert e0["step_is_valid"] == 1 and e0["step_is_successful"] == 1, (where, si)
        assert _bits(e0["trust_region_radius"]) == _bits(o.initial_trust_region_radius), (where, si)
        run = 0  # length of the current run of non-successful entries
        last_ok = e0
        for k in range(1, len(s)):
            e, prev = s[k], s[k - 1]
            tag = (where, si, k)
            if e["step_is_successful"]:
                assert e["step_is_valid"] == 1, tag
                rho = float(e["relative_decrease"])
                assert rho > o.min_relative_decrease, tag
                q = 2.0 * rho - 1.0
                want = min(o.max_trust_region_radius, float(prev["trust_region_radius"]) / max(1.0 / 3.0, 1.0 - q * q * q))
                assert abs(float(e["trust_region_radius"]) - want) <= 1e-15 * want, tag
                run = 0
                last_ok = e
                continue
            run += 1
            assert _bits(e["trust_region_radius"]) == _bits(float(prev["trust_region_radius"]) / 2.0 ** run), tag
            assert _bits(e["gradient_max_norm"]) == _bits(prev["gradient_max_norm"]), tag
            if e["step_is_valid"]:
                n_rej += 1
                assert e["relative_decrease"] <= o.min_relative_decrease, tag
            else:
                n_inv += 1
                assert e["cost_change"] == 0.0 and e["step_norm"] == 0.0 and e["relative_decrease"] == 0.0, tag
                assert _bits(e["cost"]) == _bits(last_ok["cost"]), tag
    if solves:
        assert _bits(solves[0][0]["cost"]) == _bits(rep["initial_cost"]), where
        last_ok = [e for e in solves[-1] if e["step_is_successful"]][-1]
        assert _bits(last_ok["cost"]) == _bits(rep["final_cost"]), where
    steps = log[log["iteration"] >= 1]
    assert int((steps["step_is_successful"] == 1).sum()) == rep["successful_steps"], where
    # at most one uncounted terminating iteration per solve (limo_hip.h: iterations_total counts it, the log has no entry)
    assert rep["iterations_total"] - rep["num_solves"] <= len(steps) <= rep["iterations_total"], (where, len(steps), rep["iterations_total"])
    return {"rejected": n_rej, "invalid": n_inv}


def drop_discarded(log):
    """The solves the oracle prints: it prints the retry in place of a discarded first attempt."""
    solves = split_solves(log)
    return [s for i, s in enumerate(solves) if not (int(s[0]["solve_kind"]) == 0 and i + 1 < len(solves) and int(solves[i + 1][0]["solve_kind"]) == 1)]


def check_against_oracle(log, table, where=""):
    """B, C, P against the oracle's table.  Exact: the sequence of (final solve or not, iteration, valid, successful).  cost: TOL.
    trust_region_radius where the update is exact (the oracle's rho >= 1: x 3; rejected or invalid: / 2^k): the 4 printed digits -
    the same text while every update of the solve so far was exact, else within half a unit of the fourth digit (5e-4) + TOL.
    Returns the largest relative differences of the fields that have no bar, over iterations <= 3."""
    ours = drop_discarded(log)
    assert len(ours) == len(table), (where, len(ours), len(table))
    seen = {"cost_change": 0.0, "gradient_max_norm": 0.0, "step_norm": 0.0, "relative_decrease": 0.0}
    for si, (s, t) in enumerate(zip(ours, table)):
        kind = int(s[0]["solve_kind"])
        assert (kind == 2) == (si == len(table) - 1), (where, si, kind)
        assert [(int(e["iteration"]), int(e["step_is_valid"]), int(e["step_is_successful"])) for e in s] == \
               [(r["iteration"], r["step_is_valid"], r["step_is_successful"]) for r in t], (where, si)
        exact_so_far = True
        for k, (e, r) in enumerate(zip(s, t)):
            tag = (where, si, k)
            assert abs(float(e["cost"]) - r["cost"]) <= TOL * abs(r["cost"]), tag + (float(e["cost"]), r["cost"])
            if k >= 1:
                exact = (not r["step_is_successful"]) or r["relative_decrease"] >= 1.0
                if exact:
                    if exact_so_far:
                        assert "%.3e" % float(e["trust_region_radius"]) == r["radius_text"], tag + (float(e["trust_region_radius"]), r["radius_text"])
                    else:
                        assert abs(float(e["trust_region_radius"]) - r["trust_region_radius"]) <= (5e-4 + TOL) * r["trust_region_radius"], tag
                exact_so_far = exact_so_far and exact
                if k <= 3:
                    for f in seen:
                        if r[f] != 0.0:
                            seen[f] = max(seen[f], abs(float(e[f]) - r[f]) / abs(r[f]))
    return seen


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "oracle":
        _oracle_child(sys.argv[2])
    else:
        sys.exit("usage: iteration_log_common.py oracle NAME")
