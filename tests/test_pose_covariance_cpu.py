"""Marginal pose covariance, CPU tier: the emulator runs the schedule and then the covariance pass with the kernel's own statement
(kba_items.hpp:cam_cov, tests/cpp/emu_pose_cov.cpp) and is held to the dense reference of tests/pose_cov_common.py; the reference is
held to making a difference (sensitivity), and cam_cov alone runs on hand-made systems in a stand-alone program, plain and under
the sanitizers."""
import math
import subprocess

import numpy as np
import pytest

import iteration_log_common as ilc
import lm_step_common as lsc
import pose_cov_common as pcc
from limo_amd import _ffi, default_options

OK_CASES = [n for n in pcc.cases() if pcc.expected_status(n) == pcc.OK]


@pytest.mark.parametrize("name", OK_CASES)
def test_emulator_against_the_dense_reference(name):
    w0, final, rep, cov, status, trimmed = pcc.emu_case(name)
    ref = pcc.reference(name, final, trimmed)
    assert ref.cond <= 1.3e8 * 1.05, (name, ref.cond)  # (a worse conditioned case is ill-conditioned input: another seed)
    dev = pcc.check_ok(cov, status, ref, where=name)
    print(name, "block %.2e full %.2e" % (dev["block"], dev["full"]))


def test_trimmed_cases_trim_and_the_rule_finds_their_rows():
    for seed, n_trimmed in zip(pcc.TRIMMED_SEEDS, (10, 22)):
        name = "trimmed_%d" % seed
        w0, final, rep, cov, status, trimmed = pcc.emu_case(name)
        assert len(trimmed) == n_trimmed == rep["n_trimmed_landmarks"], (name, len(trimmed))
        ref = pcc.reference(name, final, trimmed)
        assert ref.rows_obs <= ref.n_rows_removed <= ref.rows_obs + int((w0.lm_is_ground[trimmed] != 0).sum())
        # a pass that ignored lm_state would compute this one: it is 2-3e-2 away, nine decades above the bar
        untrimmed = pcc.Reference(w0, final, default_options(), trimmed=())
        far = pcc.deviation(untrimmed.cov, ref.cov, ref.free)
        assert far["full"] > 1e-2 and far["block"] > 1e-2, (name, far)
        miss = pcc.deviation(cov, untrimmed.cov, ref.free)
        assert min(miss.values()) > 100 * max(pcc.BARS.values()), (name, miss)


def test_rank_deficient_window():
    name = "shape_%d" % pcc.RANK_DEFICIENT_SEED
    w0, final, rep, cov, status, trimmed = pcc.emu_case(name)
    assert status == pcc.RANK_DEFICIENT
    assert np.isnan(cov).all()
    assert pcc.reference(name, final, trimmed).rank_deficient  # (the reference sees it too: a free keyframe without a view)


def test_window_without_a_free_pose_block():
    w0, final, rep, cov, status, trimmed = pcc.emu_case("fixed_" + pcc.NOTHING_VARIABLE)
    assert status == pcc.NO_FREE_POSE
    assert cov.shape == (6 * w0.n_kf, 6 * w0.n_kf) and not cov.any()


def test_bars_are_100x_the_cpu_spread():
    worst = {}
    for name in OK_CASES:
        w0, final, rep, cov, status, trimmed = pcc.emu_case(name)
        dev = pcc.check_ok(cov, status, pcc.reference(name, final, trimmed), bars=None, where=name)
        for cls, v in dev.items():
            if v > worst.get(cls, (0.0, ""))[0]:
                worst[cls] = (v, name)
    print("CPU spread:", {k: "%.2e (%s)" % v for k, v in worst.items()})
    for cls, bar in pcc.BARS.items():
        assert bar <= pcc.MAX_BAR, cls
        digit = bar / 10 ** math.floor(math.log10(bar))
        assert abs(digit - round(digit)) < 1e-9, (cls, "one digit", bar)
        assert worst[cls][0] <= 2 * bar / 100, (cls, "the spread has outgrown the bar", worst[cls], bar)


# ------------------------------------------------------------------------------------------------ sensitivity of the reference
SENSITIVITY_CASES = ("shape_7102", "shape_7400", "pose_71", "fixed_b")


def _misses(name, wrong):
    w0, final, rep, cov, status, trimmed = pcc.emu_case(name)
    ref = pcc.reference(name, final, trimmed)
    miss = pcc.deviation(cov, wrong.cov, ref.free)
    assert min(miss.values()) > 100 * max(pcc.BARS.values()), (name, miss)
    return miss


@pytest.mark.parametrize("name", SENSITIVITY_CASES)
def test_reference_with_damping_left_on_misses(name):
    w0, o, problem = pcc.case(name)
    final = pcc.emu_case(name)[1]
    print(name, _misses(name, pcc.Reference(w0, final, o, problem, damping=(1e4, o))))


@pytest.mark.parametrize("name", SENSITIVITY_CASES)
def test_reference_without_the_loss_correction_misses(name):
    w0, o, problem = pcc.case(name)
    final = pcc.emu_case(name)[1]
    plain = _ffi.BaOptions.from_buffer_copy(o)
    plain.depth_thres, plain.reprojection_thres = 1e9, 1e9  # rho' = 1 on every depth and reprojection row
    print(name, _misses(name, pcc.Reference(w0, final, plain, problem)))


@pytest.mark.parametrize("name", SENSITIVITY_CASES)
def test_reference_with_the_scale_not_undone_misses(name):
    w0, o, problem = pcc.case(name)
    assert o.jacobi_scaling == 1
    final = pcc.emu_case(name)[1]
    print(name, _misses(name, pcc.Reference(w0, final, o, problem, keep_scale=True)))


# ------------------------------------------------------------------------------------------------ the pass is invisible
@pytest.mark.parametrize("name", ("shape_7102", "trimmed_7400", "pose_71", "fixed_b"))
def test_pass_changes_nothing_of_the_solve(name):
    w0, o, problem = pcc.case(name)
    final, rep = pcc.emu_case(name)[1:3]
    plain = w0.copy()
    flags = None if problem.lm_fixed is None else [problem.flags(plain.n_lm)]
    reps, _ = ilc.emu_solve([plain], o, pose_only=problem.pose_only, prior=problem.prior, lm_fixed=flags)
    assert lsc.same_bytes(plain, final), name
    assert reps[0] == rep, (name, reps[0], rep)


def test_streaming_schedule_gives_the_same_bytes():
    names = ("shape_7102", "shape_7103", "shape_7400")
    ws = [pcc.case(n)[0] for n in names]
    _, mats, status, _ = pcc.emu_solve(ws, pcc.no_trim_options(), n_slots=2)
    for n, m, s in zip(names, mats, status):
        assert s == pcc.OK and m.tobytes() == pcc.emu_case(n)[3].tobytes(), n


# ------------------------------------------------------------------------------------------------ cam_cov alone
def test_standalone_host_check_plain_and_sanitized():
    for exe in pcc.build():
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "all checks passed" in p.stdout, (exe, p.stdout[-2000:], p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------ the drivers on a backend without the symbols
def test_drive_on_a_backend_without_the_symbols(tmp_path):
    """apps/limo_stream --covariance on the emulated C-ABI, which does not export the three symbols: the shim's weak references are
    null, the pose rows are those of the plain drive and every row of the covariance file says LIMO_COV_NOT_COMPUTED with zeros."""
    import emu_ffi

    exe = emu_ffi.build_stream_app()
    base = [exe, "--frames", "12", "--az", "2000", "--seed", "7", "--quiet"]
    plain, with_cov, cov = str(tmp_path / "plain.txt"), str(tmp_path / "with.txt"), str(tmp_path / "cov.txt")
    for args in (["--poses", plain], ["--poses", with_cov, "--covariance", cov]):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert open(plain, "rb").read() == open(with_cov, "rb").read()
    rows = [l.split() for l in open(cov).read().splitlines()]
    assert len(rows) == 12 and all(len(r) == 37 and int(r[36]) == pcc.NOT_COMPUTED and not any(float(x) for x in r[:36]) for r in rows)
