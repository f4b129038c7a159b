"""The per-iteration solver log (include/limo_hip.h:limo_ba_iteration) in the CPU tier: the recording of kba_lm.hpp driven by hand
(tests/cpp/test_iteration_log.cpp, also under -fsanitize=address,undefined), the emulated pipeline's logs of the four test windows
(iteration_log_common.window) on both of its schedules, their identities, and the oracle's own table for the windows whose iteration
count the oracle itself keeps under one-ulp input changes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import iteration_log_common as ilc
from limo_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_state_machine_records_what_ceres_would_push(which):
    plain, san = ilc.build_unit()
    r = subprocess.run([plain if which == "plain" else san], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout


@pytest.fixture(scope="module")
def emu_logs():
    """name -> (report, log) of the emulator's lock-step schedule; ("stream", name) -> the same from the streaming schedule, where the
    three solve windows share one batch [A, B, C, B, A] with two slots."""
    out = {}
    for name in ilc.NAMES:
        w, prior = ilc.window(name)
        reps, logs = ilc.emu_solve([w.copy()], ilc.options(name), pose_only=name == "P", prior=prior)
        out[name] = (reps[0], logs[0])
    order = ["A", "B", "C", "B", "A"]
    reps, logs = ilc.emu_solve([ilc.window(k)[0].copy() for k in order], ilc.options("A"), n_slots=2)
    out["stream"] = [(k, r, l) for k, r, l in zip(order, reps, logs)]
    w, prior = ilc.window("P")
    reps, logs = ilc.emu_solve([w.copy()], ilc.options("P"), pose_only=True, prior=prior, n_slots=1)
    out["stream"].append(("P", reps[0], logs[0]))
    return out


def test_both_schedules_of_the_emulator_give_the_same_bytes(emu_logs):
    seen = set()
    for name, rep, log in emu_logs["stream"]:
        want_rep, want = emu_logs[name]
        assert len(log) == len(want) and log.tobytes() == want.tobytes(), name
        assert all(rep[k] == want_rep[k] for k in rep if k != "time_sec"), name
        seen.add(name)
    assert seen == set(ilc.NAMES)


@pytest.mark.parametrize("name", ilc.NAMES)
def test_log_identities(emu_logs, name):
    rep, log = emu_logs[name]
    counts = ilc.check_consistency(log, rep, ilc.options(name), name)
    kinds = sorted({int(k) for k in log["solve_kind"]})
    print(name, "entries", len(log), "kinds", kinds, counts)
    assert len(log) > 0
    if name == "A":  # no trimming, rejected steps (the oracle has seven)
        assert kinds == [2] and counts["rejected"] >= 1
    else:  # a trimming solve that reduced the cost, then the final solve
        assert kinds == [0, 2]


@pytest.mark.parametrize("name", ilc.ORACLE_NAMES)
def test_oracle_comparison_windows_are_stable(name):
    lo, hi = ilc.oracle_iterations_stable(name, n=8)
    assert lo == hi, (name, lo, hi)


@pytest.mark.parametrize("name", ilc.ORACLE_NAMES)
def test_log_agrees_with_the_oracle_table(emu_logs, name):
    table, rep_o = ilc.oracle_table(name)
    rep, log = emu_logs[name]
    assert sum(len(t) for t in table) > 0
    seen = ilc.check_against_oracle(log, table, name)
    print(name, "largest relative difference to the oracle on iterations <= 3 (no bar):", {k: "%.2e" % v for k, v in seen.items()})
    assert rep["num_solves"] == rep_o["num_solves"]


def test_symbols_and_struct_size_match_the_header():
    src = open(os.path.join(ROOT, "include", "limo_hip.h")).read()
    body = re.search(r"typedef struct limo_ba_iteration \{(.*?)\} limo_ba_iteration;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "uint8_t": 1, "double": 8}
    fields, total = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            fields.append(m.group(1))
            total += sizes[ty] * int(m.group(2) or 1)
    assert total == 64 == C.sizeof(_ffi.BaIteration) == _ffi.iteration_dtype().itemsize
    assert fields == [n for n, _ in _ffi.BaIteration._fields_] == list(_ffi.iteration_dtype().names)
    for (n, _), off in zip(_ffi.BaIteration._fields_, (_ffi.iteration_dtype().fields[k][1] for k in _ffi.iteration_dtype().names)):
        assert getattr(_ffi.BaIteration, n).offset == off, n
    lib = _ffi.load()
    for sym in ("limo_ctx_set_iteration_log", "limo_ba_batch_iteration_log", "limo_ctx_last_iteration_log"):
        assert re.search(r"\bint %s\(" % sym, src), sym
        assert hasattr(lib, sym) and sym in _ffi.ABI_SYMBOLS, sym
    assert re.search(r"#define LIMO_ABI_VERSION 6\b", src)
    # NULL arguments are an error, not a crash (no context is needed to say so)
    n = C.c_int32(7)
    assert lib.limo_ctx_set_iteration_log(None, 1) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_ctx_last_iteration_log(None, 0, 0, None, C.byref(n)) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_ba_batch_iteration_log(None, 0, 0, None, C.byref(n)) == _ffi.LIMO_ERR_INVALID
