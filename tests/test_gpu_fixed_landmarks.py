"""Windowed solve with constant landmarks on the GPU: limo_ba_solve_fixed_landmarks / limo_ba_batch_create_fixed_landmarks through
the C-ABI of liblimo_hip.so against the oracle with the flagged landmarks' parameter blocks set constant
(tests/cpp/fixed_lm_ref.cpp).  The bar is fuzz_common.check_parity (identical trimmed sets, 1e-4 on cost and keyframe
translations, never the iteration-cap clause); the shapes are fixed_lm_common.shapes (tests/test_fixed_landmarks_cpu.py lists them)."""
import ctypes as C

import numpy as np
import pytest

import fixed_lm_common as flc
import fuzz_common as fc
from limo_amd import _ffi, ba, default_options

pytestmark = pytest.mark.gpu

SHAPES = flc.shapes()
PATH_SWITCHES = ("KBA_NO_COOP_SOLVE", "KBA_NO_WG_SOLVE", "KBA_STREAM_MIN", "KBA_COOP_MAX_WIN", "KBA_GROUPS", "KBA_COOP_TIMEOUT_MS")
REPORT_KEYS = ("termination", "num_solves", "iterations_total", "iterations_final", "successful_steps", "num_linearizations",
               "n_depth_blocks", "n_repr_blocks", "n_gp_blocks", "n_trimmed_landmarks", "initial_cost", "final_cost")


def _force(monkeypatch, path):
    """The launch path of the next solves, the way tests/test_gpu_ba.py forces them (None: the library's own choice)."""
    for k in PATH_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if path in ("STREAMING", "LOCKSTEP"):
        monkeypatch.setenv("KBA_NO_COOP_SOLVE", "1")
        monkeypatch.setenv("KBA_NO_WG_SOLVE", "1")
        monkeypatch.setenv("KBA_STREAM_MIN", "1" if path == "STREAMING" else "100000")
    elif path == "COOP":
        monkeypatch.setenv("KBA_NO_WG_SOLVE", "1")


def _state(b, reps):
    return [(tuple(r[k] for k in REPORT_KEYS), w.kf_pose.copy(), w.kf_plane_dir.copy(), w.kf_plane_dist.copy(), w.lm_pos.copy(), b.trimmed(i))
            for i, (w, r) in enumerate(zip(b.windows, reps))]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], (what, i, dict(zip(REPORT_KEYS, x[0])), dict(zip(REPORT_KEYS, y[0])))
        assert all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:])), (what, i)


def _solve_batch(ctx, windows, flag_list, o):
    b = ba.Batch(ctx, [w.copy() for w in windows], lm_fixed=flag_list)
    b.solve(o)
    reps = b.download()
    return b, reps


@pytest.fixture(scope="module")
def ref_results():
    o = default_options()
    out = {}
    for name, (w, flags) in SHAPES.items():
        wo = w.copy()
        ro, to = flc.ref_solve(wo, flags, o)
        out[name] = (ro, to, wo)
    return out


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_match_the_oracle_with_constant_blocks(ctx, ref_results, name, monkeypatch):
    _force(monkeypatch, None)
    w, flags = SHAPES[name]
    o = default_options()
    ro, to, wo = ref_results[name]
    wg = w.copy()
    rg = ctx.solve(wg, o, lm_fixed=flags)
    b, (rb,) = _solve_batch(ctx, [w], [flags], o)  # (the resident form of the same call: it can tell which landmarks were trimmed)
    tg = b.trimmed(0)
    assert all(rg[k] == rb[k] for k in REPORT_KEYS) and np.array_equal(wg.kf_pose, b.windows[0].kf_pose) and np.array_equal(wg.lm_pos, b.windows[0].lm_pos)
    b.close()
    so = lambda p, oo: flc.ref_solve(p, flags, oo)[0]
    sg = lambda p, oo: ctx.solve(p, oo, lm_fixed=flags)
    ok, detail, clause = flc.check_parity(w, rg, wg, tg, sg, ro, wo, to, so)
    print("%s: %s; final cost %.9g / %.9g, iterations %d / %d" % (name, detail, rg["final_cost"], ro["final_cost"], rg["iterations_total"], ro["iterations_total"]))
    assert ok, "%s: %s" % (name, detail)
    assert clause != fc.BY_CAP
    cst = flags != 0
    assert np.array_equal(wg.lm_pos[cst], w.lm_pos[cst])  # constant landmarks come back bit for bit
    assert abs(rg["initial_cost"] - ro["initial_cost"]) <= 1e-12 * abs(ro["initial_cost"])
    if name == "f":  # nothing to optimise
        for k in REPORT_KEYS[:10]:
            assert rg[k] == ro[k], k
        assert rg["termination"] == _ffi.LIMO_CONVERGENCE and rg["iterations_total"] == 0 and rg["initial_cost"] == rg["final_cost"]
        assert abs(rg["final_cost"] - ro["final_cost"]) <= 1e-12 * ro["final_cost"] and np.array_equal(wg.kf_pose, w.kf_pose)


def test_mixed_batch_equals_the_single_calls_on_every_launch_path(ctx, monkeypatch):
    """The 48-window sweep (flag densities 0.1 / 0.5 / 1.0 or no flags, drawn per window) as ONE batch with mixed NULL and non-NULL
    entries: every window bit-identical to its single call, through the streaming and the lock-step sequence, after a reset, and -
    for the windows the cooperative kernel serves (at most four free keyframes, one camera; with the small shapes, the all-constant
    (f) among them) - through k_solve_coop."""
    o = default_options()
    sw = flc.sweep(48)
    ws, fl = [w for _, w, _ in sw], [f for _, _, f in sw]
    assert any(f is None for f in fl) and any(f is not None and f.all() for f in fl) and any(f is not None and not f.all() for f in fl)
    _force(monkeypatch, None)
    single = []
    for w, f in zip(ws, fl):
        b, reps = _solve_batch(ctx, [w], [f], o)
        single += _state(b, reps)
        b.close()
    for path in ("STREAMING", "LOCKSTEP"):
        _force(monkeypatch, path)
        b, reps = _solve_batch(ctx, ws, fl, o)
        assert ctx.last_solve_info()["path"] == path
        _assert_same(_state(b, reps), single, path)
        b.reset()  # ... and once more from the reset state (lm_state 2 is part of it)
        b.solve(o)
        assert ctx.last_solve_info()["path"] == path
        _assert_same(_state(b, b.download()), single, path + " after reset")
        b.close()
    fast = [i for i, (kw, _, _) in enumerate(sw) if kw["n_kf"] <= 5 and kw["stereo_baseline"] == 0.0]
    names = ("a", "b", "c2", "c3", "d", "f", "h_b_02", "h_d_3")
    cw, cf = [ws[i] for i in fast] + [SHAPES[k][0] for k in names], [fl[i] for i in fast] + [SHAPES[k][1] for k in names]
    _force(monkeypatch, "LOCKSTEP")
    b, reps = _solve_batch(ctx, cw, cf, o)
    assert ctx.last_solve_info()["path"] == "LOCKSTEP"
    want = _state(b, reps)
    b.close()
    _assert_same(want[: len(fast)], [single[i] for i in fast], "subset")
    _force(monkeypatch, "COOP")
    b, reps = _solve_batch(ctx, cw, cf, o)
    info = ctx.last_solve_info()
    assert info["path"] == "COOP" and info["recovered"] == 0, info
    _assert_same(_state(b, reps), want, "COOP")
    b.close()


def test_no_schur_launch_without_a_variable_landmark(ctx, monkeypatch):
    """A batch whose landmarks are all constant has no Schur block: the launch sequences count no Schur launch
    (limo_ba_batch_kernel_time(LIMO_KERNEL_SCHUR)), and its own path - one workgroup per window - gives the same bits."""
    o = default_options()
    ws = [SHAPES[k][0] for k in ("e_all", "a", "c3", "f")]
    fl = [np.ones(w.n_lm, np.uint8) for w in ws]
    results = []
    for path in ("LOCKSTEP", "STREAMING", None):
        _force(monkeypatch, path)
        b, reps = _solve_batch(ctx, ws, fl, o)
        assert ctx.last_solve_info()["path"] == (path or "WG")
        st = b.kernel_stats()
        assert st["schur_launches"] == 0 and st["schur_ms"] == 0.0, st
        assert (st["linearize_launches"] > 0) == (path is not None), st
        assert any(r["iterations_total"] > 0 for r in reps)
        results.append(_state(b, reps))
        b.close()
    _assert_same(results[1], results[0], "STREAMING")
    _assert_same(results[2], results[0], "WG")
    # (the control: the same windows with variable landmarks do launch Schur kernels)
    _force(monkeypatch, "LOCKSTEP")
    b, _ = _solve_batch(ctx, ws[:3], None, o)
    assert b.kernel_stats()["schur_launches"] > 0
    b.close()


def test_null_flags_are_limo_ba_solve_bit_for_bit(ctx, monkeypatch):
    _force(monkeypatch, None)
    o = default_options()
    for name in ("a", "b", "c3", "e3"):
        w = SHAPES[name][0]
        wp = w.copy()
        rp = ctx.solve(wp, o)
        for flags in (None, np.zeros(w.n_lm, np.uint8)):
            wf = w.copy()
            s, rep = wf.as_struct(), _ffi.BaReport()
            p = None if flags is None else flags.ctypes.data_as(_ffi.c_uint8_p)
            assert ctx.lib.limo_ba_solve_fixed_landmarks(ctx.ptr, C.byref(s), p, C.byref(o), C.byref(rep)) == _ffi.LIMO_OK
            rf = rep.as_dict()
            assert all(rf[k] == rp[k] for k in REPORT_KEYS), (name, rf, rp)
            for fld in ("kf_pose", "kf_plane_dir", "kf_plane_dist", "lm_pos"):
                assert np.array_equal(getattr(wf, fld), getattr(wp, fld)), (name, fld)
    ws = [SHAPES[k][0] for k in ("a", "b", "c3", "e3")]
    b0, r0 = _solve_batch(ctx, ws, None, o)
    b1, r1 = _solve_batch(ctx, ws, [None, np.zeros(ws[1].n_lm, np.uint8), None, None], o)
    _assert_same(_state(b1, r1), _state(b0, r0), "batch without a flag set")
    b0.close()
    b1.close()


def test_invalid_input_behaves_as_limo_ba_batch_create(ctx):
    from limo_amd.window import struct_array

    w = SHAPES["a"][0].copy()
    arr = struct_array([w])
    out = C.c_void_p()
    lib = ctx.lib
    for n in (0, -3):
        assert lib.limo_ba_batch_create_fixed_landmarks(ctx.ptr, n, arr, None, C.byref(out)) == lib.limo_ba_batch_create(ctx.ptr, n, arr, C.byref(out)) != _ffi.LIMO_OK
        assert not out.value
    assert lib.limo_ba_batch_create_fixed_landmarks(ctx.ptr, 1, arr, None, None) == lib.limo_ba_batch_create(ctx.ptr, 1, arr, None) != _ffi.LIMO_OK
    assert lib.limo_ba_batch_create_fixed_landmarks(None, 1, arr, None, C.byref(out)) == lib.limo_ba_batch_create(None, 1, arr, C.byref(out)) != _ffi.LIMO_OK
    assert lib.limo_ba_solve_fixed_landmarks(ctx.ptr, None, None, None, None) == lib.limo_ba_solve(ctx.ptr, None, None, None) != _ffi.LIMO_OK
    with pytest.raises(ValueError):
        ba.Batch(ctx, [w], lm_fixed=[np.zeros(w.n_lm + 1, np.uint8)])
    with pytest.raises(ValueError):
        ba.Batch(ctx, [w], pose_only=True, lm_fixed=[None])
