"""limo_landmark_select / limo_landmark_select_batch on the GPU (limo_amd/csrc/landmark_select.hip) against the host classes
(LandmarkSelector with cheirality + voxel + add-depth as StreamDriver wires them: tests/cpp/landmark_select_ref.cpp), BYTE FOR BYTE:
category, must-have bit and rejection of every landmark.  No tolerance anywhere."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import landmark_select_common as lsc
from limo_amd import _ffi, ba

pytestmark = pytest.mark.gpu

SIZES, WINDOWS, RIGS, SEEDS = (1, 2, 63, 64, 65, 300, 1500), (1, 2, 3, 12), (1, 2), (1, 2, 3)


@pytest.fixture(scope="module")
def ctx():
    c = ba.Context(0)
    yield c
    c.close()


def gen_params(n_lm, **fields):
    """Budgets that scale with the pool (a thirtieth / a twelfth / a twentieth of it), so that they bind at 300 and at 1500 landmarks."""
    f = dict(max_near=max(1, n_lm // 30), max_middle=max(1, n_lm // 12), max_far=max(1, n_lm // 20))
    f.update(fields)
    return lsc.params(add=lsc.ADD, **f)


@functools.lru_cache(maxsize=None)
def generated(n_lm, n_kf, n_cam, seed):
    """A generated pool and the checker's bytes for it (computed once, shared by the tests)."""
    pool = lsc.make_pool(1000 * seed + n_lm + n_kf, n_lm, n_kf, n_cam)
    want = lsc.ref_select(pool, gen_params(n_lm))
    want.setflags(write=False)
    return pool, want


def same(got, want, where):
    assert got.tobytes() == want.tobytes(), (where, np.nonzero(got != want)[0][:10], got[got != want][:10], want[got != want][:10])


@pytest.mark.parametrize("n_kf", WINDOWS)
@pytest.mark.parametrize("n_lm", SIZES)
def test_single_call_equals_the_checker(ctx, n_lm, n_kf):
    for n_cam in RIGS:
        for seed in SEEDS:
            pool, want = generated(n_lm, n_kf, n_cam, seed)
            got = ctx.landmark_select(pool, gen_params(n_lm))
            same(got, want, (n_lm, n_kf, n_cam, seed))


@pytest.mark.parametrize("n_lm", [300, 1500])
def test_the_checkers_answers_are_not_empty(n_lm):
    """What keeps the comparison honest, asserted on the CHECKER's output over the generated pools of a size: all three categories, a
    must-have, a cheirality rejection, a voxel of three or more members and one of exactly two, and every budget binding in some pool (the
    checker with unlimited budgets picks more than the budget)."""
    seen, binding, vox2, vox3 = set(), set(), 0, 0
    for n_kf in WINDOWS:
        for n_cam in RIGS:
            for seed in SEEDS:
                pool, want = generated(n_lm, n_kf, n_cam, seed)
                p = gen_params(n_lm)
                seen |= set(int(b) for b in np.unique(want))
                free = lsc.ref_select(pool, lsc.with_fields(p, max_near=10**6, max_middle=10**6, max_far=10**6))
                for c, budget in ((1, p.max_near), (2, p.max_middle), (3, p.max_far)):
                    if int(((want & 3) == c).sum()) == budget < int(((free & 3) == c).sum()):
                        binding.add(c)
                sizes = lsc.voxel_sizes(pool, p, want != 8)
                vox2 += int((sizes == 2).sum())
                vox3 += int((sizes >= 3).sum())
    print("bytes seen", sorted(seen), "budgets binding", sorted(binding), "voxels of two", vox2, "of three or more", vox3)
    assert {1, 2, 3} <= set(b & 3 for b in seen if b != 8)
    assert any(b & 4 for b in seen if b != 8) and 8 in seen
    assert vox2 >= 1 and vox3 >= 1
    assert binding == {1, 2, 3}


def check(ctx, pool, p, where):
    want = lsc.ref_select(pool, p)
    same(ctx.landmark_select(pool, p), want, where)
    return want


def test_all_landmarks_in_one_voxel(ctx):
    pool = lsc.make_pool(41, 300, 3, straight=True, behind_share=0.0)
    pool["lm_pos"] = pool["centres"][-1] + np.random.default_rng(41).uniform((1.0, 0.5, 5.0), (9.0, 1.5, 30.0), (300, 3))  # one octant of the newest frame
    p = gen_params(300, voxel_size_xyz=(1000.0, 1000.0, 1000.0))
    want = check(ctx, pool, p, "one voxel")
    assert lsc.voxel_sizes(pool, p, want != 8).tolist() == [300]
    assert int(((want & 3) != 0).sum()) <= 1  # one representative (chosen if it has a flow), no far field


def test_every_landmark_in_its_own_voxel(ctx):
    pool = lsc.make_pool(42, 300, 3, double_share=0.0)
    p = gen_params(300, voxel_size_xyz=(1e-3, 1e-3, 1e-3), max_near=10**6, max_middle=10**6, max_far=10**6)
    want = check(ctx, pool, p, "own voxels")
    assert (lsc.voxel_sizes(pool, p, want != 8) == 1).all()


def pairs_pool(seed, n_pairs, n_kf):
    """Only two-member voxels: a straight drive (the newest keyframe's frame is the world shifted), pairs of landmarks around the centres
    of distinct cells inside the far pipe."""
    pool = lsc.make_pool(seed, 2 * n_pairs, n_kf, straight=True, behind_share=0.0, double_share=0.0, unseen_share=0.0)
    rng = np.random.default_rng(seed)
    cells = set()
    while len(cells) < n_pairs:
        cells.add((int(rng.integers(-20, 21)), int(rng.integers(-4, 4)), int(rng.integers(10, 100))))
    centre = (np.array(sorted(cells), np.float64) + 0.5) * np.array([0.5, 0.5, 0.3])
    rng.shuffle(centre)
    pos = np.repeat(centre, 2, axis=0)
    pos[1::2] += 0.1 * np.array([0.5, 0.5, 0.3])
    pool["lm_pos"] = pos + pool["centres"][-1]
    return pool


def test_pools_of_two_member_voxels(ctx):
    """The two members of a voxel are equidistant from their midpoint: the 1e-9 relative tie rule decides, in id order."""
    for seed, n_kf in ((1, 3), (2, 12)):
        pool = pairs_pool(seed, 150, n_kf)
        p = gen_params(300, max_near=10**6, max_middle=10**6)
        want = check(ctx, pool, p, ("pairs", seed))
        assert (lsc.voxel_sizes(pool, p, want != 8) == 2).all()
        chosen = (want & 3) != 0
        assert chosen.sum() >= 100 and not (chosen[0::2] & chosen[1::2]).any()  # at most one of a pair (a near representative needs a flow)


def test_equal_flows_and_track_lengths_go_by_id(ctx):
    pool = lsc.make_pool(43, 300, 3, n_cam=2, equal_flow=True, behind_share=0.0)
    want = check(ctx, pool, gen_params(300, max_near=7, max_far=9), "equal flows")
    near, far = np.nonzero((want & 3) == 1)[0], np.nonzero((want & 3) == 3)[0]
    assert len(near) == 7 and len(far) == 9
    free = lsc.ref_select(pool, gen_params(300, max_near=10**6, max_far=10**6))
    assert (near == np.nonzero((free & 3) == 1)[0][:7]).all() and (far == np.nonzero((free & 3) == 3)[0][:9]).all()  # the smallest ids


@pytest.mark.parametrize("budgets", [(0, 0, 0), (3, 5, 2), (10**6, 10**6, 10**6), (4294967295, 1, 0)])
def test_budgets_zero_binding_and_above_the_candidates(ctx, budgets):
    pool, _ = generated(300, 12, 2, 1)
    want = check(ctx, pool, gen_params(300, max_near=budgets[0], max_middle=budgets[1], max_far=budgets[2]), budgets)
    counts = [int(((want & 3) == c).sum()) for c in (1, 2, 3)]
    assert all(c <= b for c, b in zip(counts, budgets))
    if budgets == (3, 5, 2):
        assert counts == [3, 5, 2]
    if budgets[0] == 10**6:
        assert all(c > b for c, b in zip(counts, (3, 5, 2)))


def test_a_landmark_behind_one_camera_in_one_keyframe(ctx):
    """Camera 1 sits 2.5 m behind camera 0 along z; a landmark 2 m ahead of the newest keyframe lies behind camera 1 there and nowhere else."""
    pool = lsc.make_pool(44, 300, 3, n_cam=2, cam1_tz=-2.5, behind_share=0.0)
    i = 17
    pool["lm_pos"][i] = pool["centres"][-1] + (0.3, 0.0, 2.0)
    rows = pool["obs_lm"] == i
    for k in ("obs_kf", "obs_lm", "obs_cam", "obs_u", "obs_v", "obs_d"):  # measured by both cameras in every keyframe
        pool[k] = pool[k][~rows]
    extra = [(k, i, c) for k in range(3) for c in range(2)]
    for k, col in (("obs_kf", 0), ("obs_lm", 1), ("obs_cam", 2)):
        pool[k] = np.concatenate([pool[k], np.array([e[col] for e in extra], np.int32)])
    for k in ("obs_u", "obs_v", "obs_d"):
        pool[k] = np.concatenate([pool[k], np.full(len(extra), 100.0, np.float32)])
    p = gen_params(300)
    want = check(ctx, pool, p, "behind one camera")
    assert want[i] == 8
    keep = ~((pool["obs_lm"] == i) & (pool["obs_kf"] == 2) & (pool["obs_cam"] == 1))
    seen_less = dict(pool, **{k: pool[k][keep] for k in ("obs_kf", "obs_lm", "obs_cam", "obs_u", "obs_v", "obs_d")})
    assert check(ctx, seen_less, p, "not measured there")[i] != 8


def test_non_finite_positions_are_decided_by_the_comparisons(ctx):
    pool = lsc.make_pool(45, 300, 3, n_cam=2)
    nan, inf = float("nan"), float("inf")
    for i, (axis, v) in enumerate(((2, nan), (2, inf), (2, -inf), (0, nan), (0, inf), (1, nan), (0, -inf))):
        pool["lm_pos"][10 * i + 5, axis] = v
        pool["lm_is_ground"][10 * i + 5] = 0  # (a NaN range would be a key of the must-have sort: no strict weak order on the host)
    want = check(ctx, pool, gen_params(300, max_far=10**6), "non-finite")
    print("bytes of the non-finite landmarks", want[5:70:10])
    # NaN / inf in z, and NaN in x with a valid z (0 * NaN reaches every coordinate of the newest frame): the z cut or cheirality drops them
    assert (want[[5, 15, 25, 35]] & 7 == 0).all()


def test_a_landmark_measured_in_no_keyframe(ctx):
    pool = lsc.make_pool(46, 300, 3, unseen_share=0.0, behind_share=0.0)
    unseen = [3, 150, 299]
    keep = ~np.isin(pool["obs_lm"], unseen)
    for k in ("obs_kf", "obs_lm", "obs_cam", "obs_u", "obs_v", "obs_d"):
        pool[k] = pool[k][keep]
    want = check(ctx, pool, gen_params(300, max_near=10**6, max_middle=10**6), "unseen")
    assert (want[unseen] & 4 == 0).all() and (want[unseen] != 8).all() and (want[unseen] & 3 != 1).all()  # no must-have, no rejection, no flow


def test_must_have_frame_index_outside_the_window(ctx):
    pool, _ = generated(300, 3, 1, 2)
    add = [(3, 10, 1, 1), (-1, 10, 0, 0), (64, 10, 1, 1), (2, 4, 1, 1), (2, -3, 0, 0), (1, 0, 0, 0)]
    p = lsc.params(add=add, max_near=0, max_middle=0, max_far=0)
    want = check(ctx, pool, p, "frame_index outside")
    assert int((want & 4 != 0).sum()) == 4  # only (2, 4, ground, range) picks


def test_a_must_have_the_voxel_scheme_also_chose(ctx):
    pool, want = generated(300, 12, 1, 1)
    assert any(b in (5, 6, 7) for b in want)
    same(ctx.landmark_select(pool, gen_params(300)), want, "must-have and category")


@pytest.mark.parametrize("n_lm", [65, 300])
def test_result_does_not_depend_on_the_sort_capacity(ctx, n_lm):
    for n_kf, n_cam, seed in ((12, 1, 1), (3, 2, 2)):
        pool, want = generated(n_lm, n_kf, n_cam, seed)
        for cap in (1, 64, 65, 0):
            same(ctx.landmark_select(pool, gen_params(n_lm, sort_capacity=cap)), want, (n_lm, cap))


def test_shuffled_observation_order_gives_the_same_bytes(ctx):
    for n_lm, n_kf, n_cam, seed in ((300, 12, 2, 1), (65, 3, 1, 3), (1500, 12, 2, 2)):
        pool, want = generated(n_lm, n_kf, n_cam, seed)
        same(ctx.landmark_select(lsc.shuffled(pool, 7), gen_params(n_lm)), want, ("shuffled", n_lm))


def test_voxels_of_ten_micrometres_take_the_fallback(ctx):
    """Cell indices beyond +-2^20: the kernel flags the pool, the library finishes it with the host statement of the core header."""
    for n_lm, n_kf, n_cam in ((1, 1, 1), (65, 3, 2), (300, 12, 1)):
        pool, _ = generated(n_lm, n_kf, n_cam, 1)
        check(ctx, pool, gen_params(n_lm, voxel_size_xyz=(1e-5, 1e-5, 1e-5)), ("fallback", n_lm))


def test_ragged_batch_equals_single_calls(ctx):
    spec = [(0, 3), (1, 2), (65, 3), (300, 12), (1500, 12), (300, 0), (64, 1)]
    pools = [lsc.make_pool(900 + i, n_lm, n_kf, 1 + i % 2) for i, (n_lm, n_kf) in enumerate(spec)]
    far = lsc.make_pool(950, 300, 3)  # one pool 3000 km from the origin of the voxel grid's packed range: its cells leave +-2^20
    far["lm_pos"][:, 0] += 3.0e6
    far["kf_pose"][:, 4:] = np.array([-lsc.quat_R(q[:4]) @ (c + (3.0e6, 0, 0)) for q, c in zip(far["kf_pose"], far["centres"])])
    pools.insert(4, far)
    p = gen_params(300)
    want = [lsc.ref_select(w, p) for w in pools]
    assert (want[4] & 3 != 0).any() and len(want[0]) == 0 and not want[6].any()
    single = [ctx.landmark_select(w, p) for w in pools]
    got = ctx.landmark_select_batch(pools, p)
    for i in range(len(pools)):
        same(single[i], want[i], ("single", i))
        same(got[i], want[i], ("batch", i))
    again = ctx.landmark_select_batch(pools, p)  # pool reuse: the same blocks, the same bytes
    assert [g.tobytes() for g in again] == [g.tobytes() for g in got]
    assert ctx.landmark_select_batch([], p) == []


def test_invalid_input_is_refused_before_any_launch(ctx):
    lib = ctx.lib
    good = lsc.make_pool(47, 50, 3, 2)
    p = gen_params(50)
    out = np.zeros(64, np.uint8)
    outp = out.ctypes.data_as(_ffi.c_uint8_p)

    def call(pool=good, prm=p, o=outp, **sizes):
        w, keep = _ffi.select_pool(pool)
        for k, v in sizes.items():
            setattr(w, k, v)
        rc = lib.limo_landmark_select(ctx.ptr, C.byref(w), None if prm is None else C.byref(prm), o)
        del keep
        return rc, lib.limo_last_error(ctx.ptr)

    def edited(**arrays):
        w = dict(good)
        for k, v in arrays.items():
            w[k] = v(good[k].copy())
        return w

    def put(i, v):
        def f(a):
            a[i] = v
            return a
        return f

    assert call()[0] == _ffi.LIMO_OK
    refused = [
        ("params null", dict(prm=None), b""),
        ("out null", dict(o=None), b"out"),
        ("lm_pos null", dict(lm_pos=None), b"lm_pos"),
        ("kf_stamp null", dict(kf_stamp=None), b"kf_stamp"),
        ("obs_u null", dict(obs_u=None), b"obs_"),
        ("n_lm negative", dict(n_lm=-1), b"n_lm"),
        ("n_obs negative", dict(n_obs=-1), b"n_obs"),
        ("n_kf negative", dict(n_kf=-1), b"n_kf"),
        ("n_cam negative", dict(n_cam=-1), b"n_cam"),
        ("obs_kf out of range", dict(pool=edited(obs_kf=put(7, 3))), b"obs_kf"),
        ("obs_lm negative", dict(pool=edited(obs_lm=put(7, -1))), b"obs_lm"),
        ("obs_lm out of range", dict(pool=edited(obs_lm=put(7, 50))), b"obs_lm"),
        ("obs_cam out of range", dict(pool=edited(obs_cam=put(7, 2))), b"obs_cam"),
        ("lm_id not ascending", dict(pool=edited(lm_id=put(20, good["lm_id"][19]))), b"lm_id"),
        ("duplicate observation", dict(pool=edited(obs_kf=put(1, good["obs_kf"][0]), obs_lm=put(1, good["obs_lm"][0]), obs_cam=put(1, good["obs_cam"][0]))), b"duplicate"),
        ("voxel zero", dict(prm=gen_params(50, voxel_size_xyz=(0.5, 0.0, 0.3))), b"voxel"),
        ("voxel negative", dict(prm=gen_params(50, voxel_size_xyz=(-0.5, 0.5, 0.3))), b"voxel"),
        ("voxel nan", dict(prm=gen_params(50, voxel_size_xyz=(0.5, 0.5, float("nan")))), b"voxel"),
        ("roi_far zero", dict(prm=gen_params(50, roi_far=0.0)), b"roi_far"),
        ("roi_middle negative", dict(prm=gen_params(50, roi_middle=-1.0)), b"roi_middle"),
        ("n_kf 65", dict(pool=lsc.make_pool(48, 50, 65)), b"n_kf"),
        ("n_cam 9", dict(pool=lsc.make_pool(49, 50, 3, 9)), b"n_cam"),
        ("sort_capacity negative", dict(prm=gen_params(50, sort_capacity=-1)), b"sort_capacity"),
        ("unknown predicate", dict(prm=lsc.params(add=[(0, 1, 2, 0)])), b"predicate"),
    ]
    for name, kw, field in refused:
        out[:] = 77
        rc, msg = call(**kw)
        assert rc == _ffi.LIMO_ERR_INVALID, name
        assert field in msg, (name, msg)  # limo_last_error names the field ...
        if not set(kw) <= {"prm"}:
            assert b"pool 0" in msg, (name, msg)  # ... and the pool
        assert (out == 77).all(), name  # nothing was written
    assert lib.limo_landmark_select(ctx.ptr, None, C.byref(p), outp) == _ffi.LIMO_ERR_INVALID
    assert lsc.make_pool(48, 50, 64)["kf_stamp"].size == 64 and call(pool=lsc.make_pool(48, 50, 64))[0] == _ffi.LIMO_OK  # the limits themselves pass
    assert call(pool=lsc.make_pool(49, 50, 3, 8))[0] == _ffi.LIMO_OK
    # a pool of a batch: the error names it and the field
    arr = (_ffi.SelectPool * 3)()
    keep = []
    for i, w in enumerate((good, good, edited(obs_cam=put(3, 5)))):
        arr[i], k = _ffi.select_pool(w)
        keep.append(k)
    outs = [np.zeros(64, np.uint8) for _ in range(3)]
    ptrs = (_ffi.c_uint8_p * 3)(*[o.ctypes.data_as(_ffi.c_uint8_p) for o in outs])
    assert lib.limo_landmark_select_batch(ctx.ptr, 3, arr, C.byref(p), ptrs) == _ffi.LIMO_ERR_INVALID
    assert b"pool 2" in lib.limo_last_error(ctx.ptr) and b"obs_cam" in lib.limo_last_error(ctx.ptr)
    assert not any(o.any() for o in outs)
    assert lib.limo_landmark_select_batch(ctx.ptr, -1, arr, C.byref(p), ptrs) == _ffi.LIMO_ERR_INVALID
    assert lib.limo_landmark_select_batch(ctx.ptr, 3, None, C.byref(p), ptrs) == _ffi.LIMO_ERR_INVALID
    # empty pools are no error: all zero
    out[:] = 77
    assert call(pool=lsc.make_pool(50, 50, 0))[0] == _ffi.LIMO_OK and not out[:50].any()
    assert call(pool=lsc.make_pool(51, 0, 3))[0] == _ffi.LIMO_OK
    # the context is fine afterwards
    same(ctx.landmark_select(good, p), lsc.ref_select(good, p), "after the refusals")


def test_drive_with_either_selector_gives_the_same_pose_rows(tmp_path):
    import emu_ffi

    exe = emu_ffi.build_stream_app(gpu=True)
    rows, info = {}, {}
    for name, extra in (("device", ["--select-device"]), ("host", ["--select-host"]), ("default", [])):
        path = str(tmp_path / (name + ".txt"))
        r = subprocess.run([exe, "--frames", "40", "--az", "2000", "--quiet", "--poses", path] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows[name] = open(path, "rb").read()
        info[name] = {l.split()[0]: float(l.split()[1]) for l in r.stdout.splitlines() if len(l.split()) == 2 and l.split()[0].startswith(("select_", "solves", "ate_"))}
        print(name, info[name])
    assert info["device"]["select_device_calls"] >= 1 and info["device"]["select_device_calls"] == info["device"]["solves"]
    assert info["host"]["select_device_calls"] == 0 and info["default"]["select_device_calls"] == 0
    assert len(rows["device"].splitlines()) == 40
    assert rows["device"] == rows["host"] == rows["default"]
