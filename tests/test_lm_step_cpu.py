"""CPU tier of the one-step check (tests/lm_step_common.py): the emulator of the kernel pipeline and the oracle's own Schur-based
solve go through check_step on every shape and option case of the GPU tier (tests/test_gpu_lm_step.py).  These runs prove the dense
reference before any GPU run and set the bars: 100 x the largest deviation either implementation shows.  Two sensitivity tests show
that the check would catch a subtly wrong kernel: a measurement moved by 1e-3 px fails it, and every option case moves the reference
by at least 1e4 bars.

The same holds for the cases of the other problem kinds (tests/test_gpu_lm_step_kinds.py): fixed-landmark and pose-only windows on
both implementations (the oracle through tests/cpp/step_kinds_ref.cpp and pyoracle.adjust_pose_only), the landmark-sharded solve on
the emulator (no log: check_params_only).  Their sensitivity tests: one constness flag flipped, the prior's speed_weight or dt_cur
off by 1e-6, a fixed-cost block counted into the variable cost - each misses by at least 100 bars."""
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


KINDS = {"fixed": (lsc.fixed_cases, lsc.fixed_window), "pose_only": (lsc.pose_cases, lsc.pose_window), "sharded": (lsc.sharded_cases, None)}


def _kind_case_names(kind):
    """The case names of a problem kind, in the order of its case list."""
    return list(dict.fromkeys(c[0] for c in KINDS[kind][0]()))


# the runs of the other problem kinds as names of test_step_against_the_dense_reference: "<kind>:<case>"
KIND_NAMES = ["%s:%s" % (kind, c) for kind in KINDS for c in _kind_case_names(kind)]
IMPL_NAMES = [(impl, name) for impl in ("emulator", "oracle") for name in CASE_NAMES + KIND_NAMES
              if not (impl == "oracle" and name.startswith("sharded:"))]  # (the oracle has no sharded solve)


@functools.lru_cache(maxsize=None)
def _kind_runs(impl, kind, name):
    """[(window name, before, after, report, log, mid, problem)] of an implementation on the windows of a case of a problem kind
    (sharded: the window name carries the shard count and the log is None): computed once, never changed."""
    o = lsc.case_options(name)
    one = lsc.one_step_options(o) if o.max_num_iterations == 2 else None
    out = []
    for case in KINDS[kind][0]():
        if case[0] != name:
            continue
        if kind == "sharded":
            w, P = lsc.sharded_window(case[1]), case[2]
            before, after, rep = lsc.emu_run_sharded(w, o, P)
            mid = lsc.emu_run_sharded(w, one, P)[1] if one else None
            out.append(("%s/%d" % (case[1], P), before, after, rep, None, mid, lsc.SOLVE))
            continue
        w, problem = KINDS[kind][1](case[1])
        if impl == "emulator":
            before, after, rep, log = lsc.emu_run([w], o, problem)[0]
            mid = lsc.emu_run([w], one, problem)[0][1] if one else None
        else:
            before, after, rep, log = lsc.oracle_run(w, o, problem)
            mid = lsc.oracle_run(w, one, problem)[1] if one else None
        out.append((case[1], before, after, rep, log, mid, problem))
    return out


def _check(impl, name, bars):
    total = {}
    if ":" in name:
        kind, case = name.split(":")
        o = lsc.case_options(case)
        for wname, before, after, rep, log, mid, problem in _kind_runs(impl, kind, case):
            where = "%s %s %s" % (impl, name, wname)
            if log is None:
                dev = lsc.check_params_only(before, after, rep, o, mid=mid, bars=bars, where=where)
            else:
                dev = lsc.check_step(before, after, rep, log, o, mid=mid, counts_ending_iteration=impl == "emulator", bars=bars, where=where, problem=problem)
            print(impl, name, wname, {c: "%.1e" % v for c, v in dev.items()})
            lsc.merge(total, dev)
        return total
    for seed, before, after, rep, log, mid in _runs(impl, name):
        dev = lsc.check_step(before, after, rep, log, lsc.case_options(name), mid=mid, counts_ending_iteration=impl == "emulator", bars=bars,
                             where="%s %s %d" % (impl, name, seed))
        print(impl, name, seed, {c: "%.1e" % v for c, v in dev.items()})
        lsc.merge(total, dev)
    return total


@pytest.mark.parametrize("impl,name", IMPL_NAMES, ids=["%s-%s" % c for c in IMPL_NAMES])
def test_step_against_the_dense_reference(impl, name):
    _check(impl, name, lsc.BARS)


def test_bars_are_100x_the_cpu_spread():
    """The largest deviation of the emulator and the oracle from the reference over all cases of all problem kinds, per class: the
    bars are 100 x that (rounded up to one digit when they were written down; held here within a factor of two, since the last digits
    of the spread move with the host's linear algebra library), and none exceeds 1e-8."""
    spread = {}
    for impl, name in IMPL_NAMES:
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


def _kind_option_windows(name):
    """[(label, window, problem)]: the fixed-landmark and pose-only windows the option case `name` runs on."""
    out = [("fixed " + n, *lsc.fixed_window(n)) for n in lsc.FIXED_OPTION_WINDOWS if name in lsc.FIXED_OPTION_CASES]
    return out + [("pose_only " + n, *lsc.pose_window(n)) for n in lsc.POSE_OPTION_WINDOWS.get(name, ())]


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
    for label, w, problem in _kind_option_windows(name):
        d = lsc.reference_difference(w, o, base, problem)
        print(name, label, "references apart by %.1e bars" % d)
        assert d >= 1e4, (name, label, d)


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
    for label, w, problem in _kind_option_windows(name):
        lin = lsc.linearisation(w, o, problem=problem)
        n2 = (lin.Js**2).sum(0)
        clamped = (n2 < o.min_lm_diagonal) | (n2 > o.max_lm_diagonal)
        print(name, label, "clamped %d of %d columns" % (clamped.sum(), len(n2)))
        assert 0 < clamped.sum() < len(n2), (name, label)


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
    # the same flows on the fixed-landmark and pose-only windows that run these cases
    for label, w, problem in _kind_option_windows("min_relative_decrease_10"):
        r = lsc.run_reference(w, lsc.case_options("min_relative_decrease_10"), problem=problem)
        assert [e["step_is_successful"] for e in r["entries"]] == [1, 0, 0] and [e["trust_region_radius"] for e in r["entries"]] == [1e4, 5e3, 1.25e3], label
    for label, w, problem in _kind_option_windows("function_tolerance_1e3"):
        r = lsc.run_reference(w, lsc.case_options("function_tolerance_1e3"), problem=problem)
        assert len(r["entries"]) == 1 and r["termination"] == 0 and r["ended_in_decision"] and r["iterations"] == 1, label


def _kind_windows(kind):
    """[(label, window, problem)] of every window of a problem kind that runs the step cases."""
    if kind == "sharded":
        return [(n, lsc.sharded_window(n), lsc.SOLVE) for n in dict.fromkeys(c[1] for c in lsc.sharded_cases())]
    names = dict.fromkeys(c[1] for c in KINDS[kind][0]() if c[0] == "default")
    return [(n, *KINDS[kind][1](n)) for n in names]


@pytest.mark.parametrize("kind", list(KINDS))
def test_no_case_passes_by_doing_nothing(kind):
    """Every window of the other problem kinds, on the reference's numbers, scaled and unscaled: the step is valid (run_reference
    asserts mcc > 0), a one-step solve accepts it, and a two-step solve accepts both - but for the g_* family, which runs one step."""
    for label, w, problem in _kind_windows(kind):
        for one, two in (("default", "two_steps"), ("unscaled", "two_steps_unscaled")):
            r = lsc.run_reference(w, lsc.case_options(one), problem=problem)
            assert [e["step_is_successful"] for e in r["entries"]] == [1, 1] and r["entries"][1]["model_cost_change"] > 0.0, (kind, label, one)
            if label.startswith("g_"):
                continue
            r = lsc.run_reference(w, lsc.case_options(two), problem=problem)
            assert [e["step_is_successful"] for e in r["entries"]] == [1, 1, 1], (kind, label, two)


# ------------------------------------------------------------------------------------------------ what limo_hip.h says beside the step
def test_zero_speed_weight_is_no_prior_bit_for_bit():
    """A prior with speed_weight = 0 is no prior: the emulator's parameters, report and log are those of prior = None."""
    for case in lsc.KIND_STEP_CASES:
        runs = {r[0]: r for r in _kind_runs("emulator", "pose_only", case)}
        for seed in lsc.POSE_SEEDS:
            none, w0 = runs["%d_none" % seed], runs["%d_w0" % seed]
            assert lsc.same_bytes(none[2], w0[2]) and none[4].tobytes() == w0[4].tobytes() and len(none[4]) == len(w0[4]), (case, seed)
            assert {k: v for k, v in none[3].items() if k != "time_sec"} == {k: v for k, v in w0[3].items() if k != "time_sec"}, (case, seed)
        # (and the prior itself is not vacuous: with it the pose differs)
        assert not lsc.same_bytes(runs["71"][2], runs["71_none"][2]), case


def test_window_with_nothing_to_optimise():
    """Shape (f) of the fixed-landmark shapes - every block constant - has no step to hold to the reference and is held to limo_hip.h:
    LIMO_CONVERGENCE, zero iterations, no log entry, the parameters bit for bit, initial_cost == final_cost == the cost of the problem
    (all of it fixed cost) at the scalar bar."""
    from limo_amd import _ffi

    w, problem = lsc.fixed_window("f")
    for o in (lsc.case_options("default"), lsc.case_options("two_steps_unscaled")):
        assert lsc.step_probe(w, o, None, problem) is None  # the oracle takes no step either
        lsc.check_nothing_to_optimise(*lsc.emu_run([w], o, problem)[0], o, problem, where="emulator f")
        before, after, rep, log = lsc.oracle_run(w, o, problem)
        assert rep["termination"] == _ffi.LIMO_CONVERGENCE and rep["iterations_total"] == 0 and lsc.same_bytes(after, before)


# ------------------------------------------------------------------------------------------------ sensitivity of the new checks
def _worst(dev):
    return max(dev[c] / lsc.BARS[c] for c in dev)


def test_flipped_flag_fails_the_check():
    """ONE constant landmark solved as a variable one, held to the reference of the flags as given.  The landmark itself moves, which
    the bit-for-bit rule catches; put back by hand, the rest of the window - the keyframes that landmark pulls at, the scalars - is
    still off by more than 100 bars."""
    o = lsc.step_options()
    for name in ("a", "b"):
        w, problem = lsc.fixed_window(name)
        l = int(np.nonzero(problem.lm_fixed)[0][1])
        flipped = problem.lm_fixed.copy()
        flipped[l] = 0
        before, after, rep, log = lsc.emu_run([w], o, lsc.Problem(lm_fixed=flipped))[0]
        assert after.lm_pos[l].tobytes() != before.lm_pos[l].tobytes()
        with pytest.raises(AssertionError):
            lsc.check_step(before, after, rep, log, o, problem=problem, where="flipped " + name)
        after.lm_pos[l] = before.lm_pos[l]
        dev = lsc.check_step(before, after, rep, log, o, problem=problem, bars=None)
        print("flipped", name, l, {c: "%.1e" % v for c, v in dev.items()}, "%.1e bars" % _worst(dev))
        assert _worst(dev) >= 1e2


@pytest.mark.parametrize("field", ["speed_weight", "dt_cur"])
def test_perturbed_prior_fails_the_check(field):
    """The emulator's result with the prior's speed_weight / dt_cur off by a factor 1 + 1e-6, held to the reference of the prior as
    given: the speed rows carry a wrong weight / a wrong predicted motion, six digits down.
    How far 1e-6 on the weight of three rows moves a step against 20 .. 300 reprojection rows is a property of the window: on the
    reference's own numbers (the reference of the perturbed prior against that of the given one) it is 0.8 .. 63 bars on the four full
    windows and 62 on 71 cut down to 20 landmarks - no window for this test - and 420 and 1100 bars on 72 and 73 cut down, which both
    fields run on.  dt_cur also moves the position the rows pull towards and passes 100 bars on the full windows 71 and 72 as well.
    That the reference moves by 100 bars is asserted first: the implementation then has to miss by as much."""
    from limo_amd import _ffi

    o = lsc.step_options()
    for name in ("72_small", "73_small") + (("71", "72") if field == "dt_cur" else ()):
        w, problem = lsc.pose_window(name)
        p = _ffi.SpeedPrior.from_buffer_copy(problem.prior)
        setattr(p, field, getattr(p, field) * (1.0 + 1e-6))
        assert lsc.reference_difference(w, o, o, lsc.Problem("pose_only", prior=p), problem_b=problem) >= 1e2, (field, name)
        before, after, rep, log = lsc.emu_run([w], o, lsc.Problem("pose_only", prior=p))[0]
        with pytest.raises(AssertionError):
            lsc.check_step(before, after, rep, log, o, problem=problem, where="%s %s" % (field, name))
        dev = lsc.check_step(before, after, rep, log, o, problem=problem, bars=None)
        print(field, name, {c: "%.1e" % v for c, v in dev.items()}, "%.1e bars" % _worst(dev))
        assert _worst(dev) >= 1e2


def test_fixed_cost_in_the_variable_cost_fails_the_check():
    """A fixed-cost block counted into the variable cost: shape h_b_02 (keyframes 0 and 2 pose-fixed, so the blocks between them and
    the constant landmarks are fixed cost) held to the reference of the same flags with every keyframe free, whose variable cost has
    those blocks.  The relative_decrease of the step misses by more than 100 bars."""
    o = lsc.step_options()
    w, problem = lsc.fixed_window("h_b_02")
    assert lsc.linearisation(w, o, problem=problem).fixed_cost > 0.0
    before, after, rep, log = lsc.emu_run([w], o, problem)[0]
    free, _ = lsc.fixed_window("g_b")
    assert all(getattr(free, n).tobytes() == getattr(w, n).tobytes() for n, _ in w.FIELDS if n != "kf_fixation")
    with pytest.raises(AssertionError):
        lsc.check_step(free, after, rep, log, o, problem=problem, where="h_b_02 against g_b")
    ref = lsc.run_reference(free, o, problem=problem)
    assert lsc.linearisation(free, o, problem=problem).fixed_cost == 0.0 and len(ref["entries"]) == 2 == len(log)
    miss = abs(float(log[1]["relative_decrease"]) - ref["entries"][1]["relative_decrease"]) / abs(ref["entries"][1]["relative_decrease"])
    print("relative_decrease off by %.1e = %.1e bars" % (miss, miss / lsc.BARS["scalar"]))
    assert miss >= 1e2 * lsc.BARS["scalar"]
