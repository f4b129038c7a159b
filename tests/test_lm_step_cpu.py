"""CPU tier of the one-step check (tests/lm_step_common.py): the emulator of the kernel pipeline and the oracle's own Schur-based
solve go through check_step on every shape and option case of the GPU tier (tests/test_gpu_lm_step.py).  These runs prove the dense
reference before any GPU run and set the bars: 100 x the largest deviation either implementation shows.  Two sensitivity tests show
that the check would catch a subtly wrong kernel: a measurement moved by 1e-3 px fails it, and every option case moves the reference
by at least 1e4 bars."""
import functools

import numpy as np
import pytest

import iteration_log_common as ilc
import lm_step_common as lsc

CASE_NAMES = list(lsc.SHAPE_CASES) + list(lsc.OPTION_CASES)


@functools.lru_cache(maxsize=None)
def _runs(impl, name):
    """[(seed, before, after, report, log, mid)] of an implementation on the windows of a case: computed once, never changed."""
    o = lsc.case_options(name)
    seeds = [s for n, s in lsc.all_cases() if n == name]
    two = o.max_num_iterations == 2
    if impl == "emulator":
        runs = lsc.emu_run(seeds, o)
        mids = [r[1] for r in lsc.emu_run(seeds, lsc.one_step_options(o))] if two else [None] * len(seeds)
    else:
        runs = [lsc.oracle_run(s, o) for s in seeds]
        mids = [lsc.oracle_run(s, lsc.one_step_options(o))[1] if two else None for s in seeds]
    return [(s,) + r + (m,) for s, r, m in zip(seeds, runs, mids)]


def _check(impl, name, bars):
    total = {}
    for seed, before, after, rep, log, mid in _runs(impl, name):
        dev = lsc.check_step(before, after, rep, log, lsc.case_options(name), mid=mid, counts_ending_iteration=impl == "emulator", bars=bars,
                             where="%s %s %d" % (impl, name, seed))
        print(impl, name, seed, {c: "%.1e" % v for c, v in dev.items()})
        lsc.merge(total, dev)
    return total


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("impl", ["emulator", "oracle"])
def test_step_against_the_dense_reference(impl, name):
    _check(impl, name, lsc.BARS)


def test_bars_are_100x_the_cpu_spread():
    """The largest deviation of the emulator and the oracle from the reference over all cases, per class: the bars are 100 x that
    (rounded up to one digit when they were written down; held here within a factor of two, since the last digits of the spread move
    with the host's linear algebra library), and none exceeds 1e-8."""
    spread = {}
    for impl in ("emulator", "oracle"):
        for name in CASE_NAMES:
            lsc.merge(spread, _check(impl, name, None))
    print("CPU spread:", {c: "%.2e" % v for c, v in sorted(spread.items())})
    assert set(spread) == set(lsc.BARS)
    for cls, bar in lsc.BARS.items():
        assert bar <= lsc.MAX_BAR, cls
        assert 100.0 * spread[cls] <= 2.0 * bar, (cls, "spread %.3e" % spread[cls], "bar %.1e" % bar)


def test_oracle_schur_step_against_the_dense_step():
    """The probe's own y (SchurEliminator + Cholesky + back-substitution) against the refined dense y, relative to max|y|."""
    worst = 0.0
    for c in lsc.SHAPES:
        for o in (lsc.step_options(), lsc.step_options(jacobi_scaling=0)):
            lin = lsc.linearisation(c["seed"], o)
            y = lin.step(o.initial_trust_region_radius)["y"]
            worst = max(worst, float(np.abs(lin.probe_y - y).max() / np.abs(y).max()))
    print("oracle Schur y against the dense y: %.1e of max|y|" % worst)
    assert worst <= 1e-9


def test_perturbed_measurement_fails_the_check():
    """The emulator's result on a window with ONE obs_u moved by 1e-3 px, held to the reference of the unperturbed window."""
    for seed in (7102, 7303):
        o = lsc.step_options()
        before = lsc.window(seed)
        moved = before.copy()
        moved.obs_u[moved.n_obs // 2] += np.float32(1e-3)
        assert (moved.obs_u != before.obs_u).sum() == 1
        after = moved.copy()
        reps, logs = ilc.emu_solve([after], o)
        with pytest.raises(AssertionError):
            lsc.check_step(before, after, reps[0], logs[0], o, where="perturbed %d" % seed)
        dev = lsc.check_step(before, after, reps[0], logs[0], o, bars=None)
        print("perturbed", seed, {c: "%.1e" % v for c, v in dev.items()})
        assert max(dev[c] / lsc.BARS[c] for c in dev) >= 1e2  # not a near miss: the check has that much room over the bars


@pytest.mark.parametrize("name", list(lsc.OPTION_CASES))
def test_option_cases_are_not_vacuous(name):
    """The reference under the case's options against the reference under the default options (same number of steps): apart by at
    least 1e4 bars, or a different flow."""
    o = lsc.case_options(name)
    base = lsc.step_options(o.max_num_iterations)
    if name == "two_steps":  # its option is the second step: the second entry has to exist and to differ from the first
        for seed in lsc.SMALL:
            ref = lsc.run_reference(lsc.window(seed), o)
            assert [e["step_is_successful"] for e in ref["entries"]] == [1, 1, 1], seed
        return
    for seed in lsc.SMALL:
        d = lsc.reference_difference(seed, o, base)
        print(name, seed, "references apart by %.1e bars" % d)
        assert d >= 1e4, (name, seed, d)


def test_jacobi_scaling_alone_leaves_the_step_where_it_is():
    """Why jacobi_scaling = 0 is a shape run and no option case: while no column is clamped, |D y|^2 with D^2 = colnorm^2(J s) / radius
    is sum colnorm^2(J)_j delta_j^2 / radius in the unscaled variables - the same problem with or without s.  The two references agree
    within the bars; what the run holds is the kernels' other path (no scale pass, unit scale in the diagonal and the update)."""
    for c in lsc.SHAPES:
        d = lsc.reference_difference(c["seed"], lsc.case_options("unscaled"), lsc.case_options("default"))
        assert d <= 1.0, (c, d)


@pytest.mark.parametrize("name", ["min_diag", "max_diag", "min_diag_unscaled", "max_diag_unscaled"])
def test_lm_diagonal_cases_clamp_part_of_the_columns(name):
    o = lsc.case_options(name)
    for seed in lsc.SMALL:
        lin = lsc.linearisation(seed, o)
        n2 = (lin.Js**2).sum(0)
        clamped = (n2 < o.min_lm_diagonal) | (n2 > o.max_lm_diagonal)
        print(name, seed, "clamped %d of %d columns" % (clamped.sum(), len(n2)))
        assert 0 < clamped.sum() < len(n2), (name, seed)


def test_expected_flows():
    """The flows the issue's option cases are there for, on the reference's numbers."""
    for seed in lsc.SMALL:
        w = lsc.window(seed)
        flow = lambda name: lsc.run_reference(w, lsc.case_options(name))
        r = flow("min_relative_decrease_10")
        assert [e["step_is_successful"] for e in r["entries"]] == [1, 0, 0] and [e["trust_region_radius"] for e in r["entries"]] == [1e4, 5e3, 1.25e3]
        r = flow("max_radius_2e4")
        assert [e["trust_region_radius"] for e in r["entries"]] == [1e4, 2e4, 2e4] and r["entries"][1]["radius_exact"]
        for name in ("gradient_tolerance_1e9", "min_radius_1e5"):
            r = flow(name)
            assert len(r["entries"]) == 1 and r["termination"] == 0 and not r["ended_in_decision"]
        for name in ("parameter_tolerance_1e3", "function_tolerance_1e3"):
            r = flow(name)
            assert len(r["entries"]) == 1 and r["termination"] == 0 and r["ended_in_decision"] and r["iterations"] == 1
