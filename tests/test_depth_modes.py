"""The modes of mono_lidar_fusion_parameters.yaml beyond the default configuration (include/limo_hip.h ABI 6; "MODES" in
the header of limo_amd/csrc/depth.hip): radius search, PCA patch, clamping gates, ground corridor, ground-patch estimators,
the per-feature reason codes, the refused settings and the parameter file itself.

Three tiers.  (1) tests/cpp/depth_modes_ref.cpp restates the whole estimator with every mode on the CPU; with default
parameters it has to equal the frozen oracle bit for bit, and its reason counts have to equal the oracle's per-gate counts.
(2) numpy checks written from the parameter file only hold the restatement's modes on scenes with known answers.
(3) the GPU has to equal the restatement bit for bit - depths and reason codes - in every mode."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_modes_common as dm
import emu_ffi
from limo_amd import _ffi, load_depth_params, synth_lidar
from limo_amd.synth import KITTI_CX, KITTI_CY, KITTI_F
from test_depth import expected_wall_depth, wall_frame

ROOT = dm.ROOT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- interface
def test_abi_6_appends_to_the_depth_parameters():
    src = open(os.path.join(ROOT, "include", "limo_hip.h")).read()
    assert re.search(r"#define LIMO_ABI_VERSION 6\b", src) and _ffi.ABI_VERSION == 6
    assert _ffi.LIMO_ERR_UNSUPPORTED == -5 and re.search(r"LIMO_ERR_UNSUPPORTED = -5\b", src)
    # existing fields keep their offsets: ABI 5 ended with ransac_seed at byte 184 of 192
    assert _ffi.DepthParams.ransac_seed.offset == 184 and _ffi.DepthParams.neighbor_search_mode.offset == 192
    assert _ffi.DepthParams.pixelarea_search_width.offset == 0 and _ffi.DepthParams.plane_estimator_use_mestimator.offset == 176
    # the ctypes mirror lists the header's fields in the header's order
    body = re.search(r"typedef struct limo_depth_params \{(.*?)\} limo_depth_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(?:int32_t|double|uint64_t)\s+(\w+)\s*;", body)
    assert fields == [name for name, _ in _ffi.DepthParams._fields_]
    kinds = re.findall(r"\b(int32_t|double|uint64_t)\s+\w+\s*;", body)
    assert [{"int32_t": C.c_int32, "double": C.c_double, "uint64_t": C.c_uint64}[k] for k in kinds] == [t for _, t in _ffi.DepthParams._fields_]
    # enum limo_depth_reason
    enum = re.search(r"enum limo_depth_reason \{(.*?)\};", src, re.S).group(1)
    names = re.findall(r"LIMO_DEPTH_(\w+) = (\d+)", enum)
    assert [n for n, _ in names] == _ffi.DEPTH_REASON_NAMES and [int(v) for _, v in names] == list(range(10))
    assert "limo_depth_last_reasons" in _ffi.ABI_SYMBOLS and hasattr(_ffi.load(), "limo_depth_last_reasons")


def test_default_params_are_the_files_values():
    """limo_depth_default_params == the committed copy of the reference's parameter file, key by key; the two fields that
    are no keys of the file keep their values."""
    lib = _ffi.load()
    want = _ffi.DepthParams()
    lib.limo_depth_default_params(C.byref(want))
    got = load_depth_params(dm.GOLDEN_YAML)
    zero = dm.file_defaults()  # the file over a zeroed struct: every key of the struct but two is in the file
    for name, _ in _ffi.DepthParams._fields_:
        assert getattr(got, name) == getattr(want, name) == getattr(zero, name), name
    assert (want.do_use_radiusSearch, want.radiusSearch_radius, want.pca_treshold_3_2_rel_max, want.depth_segmentation_max_pointcount) == (1, 10.0, 15.0, 4)


def test_cpp_reader_equals_python_reader(tmp_path):
    exe = dm.build_params_dump()
    changed = tmp_path / "changed.yaml"
    text = open(dm.GOLDEN_YAML).read()
    text = text.replace("neighbor_search_mode: 0", "neighbor_search_mode: 1").replace("radiusSearch_radius: 10", "radiusSearch_radius: 7.25")
    text = text.replace("pixelarea_search_witdh: 6", "pixelarea_search_witdh: 11   # wider").replace("ransac_plane_min_z: -3.5", "ransac_plane_min_z: -2.75")
    changed.write_text(text)
    for path in (dm.GOLDEN_YAML, str(changed)):
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        p = load_depth_params(path, _ffi.DepthParams())
        assert r.stdout.strip() == bytes(p).hex()
    p = load_depth_params(str(changed))
    assert (p.neighbor_search_mode, p.radiusSearch_radius, p.pixelarea_search_width, p.ransac_plane_min_z) == (1, 7.25, 11, -2.75)
    # keys absent from the file keep their defaults
    short = tmp_path / "short.yaml"
    short.write_text("%YAML:1.0\n\n# only one key\ndo_use_PCA: 1\n")
    p = load_depth_params(str(short))
    assert p.do_use_PCA == 1 and p.pixelarea_search_height == 9 and p.ransac_seed == 1
    # an unknown key or a value that does not parse is an error that names the line, in both readers
    for bad, line, what in (("do_use_PCA: 1\nno_such_key: 3\n", 2, "no_such_key"), ("\n\nradiusSearch_radius: ten\n", 3, "radiusSearch_radius"),
                            ("do_use_PCA: 1.5\n", 1, "do_use_PCA"), ("pixelarea_search_width: 6\n", 1, "pixelarea_search_width"), ("do_use_PCA\n", 1, "do_use_PCA")):
        f = tmp_path / "bad.yaml"
        f.write_text(bad)
        with pytest.raises(ValueError, match=r"bad\.yaml:%d: .*%s" % (line, what)):
            load_depth_params(str(f))
        r = subprocess.run([exe, str(f)], capture_output=True, text=True)
        assert r.returncode == 2 and re.search(r"bad\.yaml:%d: .*%s" % (line, what), r.stderr), r.stderr


# ------------------------------------------------------------------------- the restatement against the frozen oracle (CPU)
def oracle_scenes():
    yield "wall", wall_frame(tilt=0.0), False
    yield "tilted wall", wall_frame(tilt=0.01), False
    yield "collinear", wall_frame(row_px=40.0), False
    yield "sparse", wall_frame(step_px=50.0, row_px=50.0), False
    near, far = wall_frame(depth=10.0, row_px=4.0), wall_frame(depth=14.0, row_px=4.0)
    two = dict(near)
    two["cloud"] = np.concatenate([near["cloud"], far["cloud"]])
    yield "two walls", two, False
    for seed in (1, 2, 4, 5, 11, 12):
        fr = synth_lidar.make_frame(seed)
        yield "sweep %d" % seed, fr, True
        if seed in (5, 11):
            yield "sweep %d without labels" % seed, fr, False


ORACLE_STATS = re.compile(r"< 3 neighbours (\d+), no histogram bin (\d+), segment < 3 (\d+), triangle not planar enough (\d+), ray \|\| plane (\d+), "
                          r"global gate (\d+), local gate (\d+), accepted (\d+)")
STATS_ORDER = [_ffi.DEPTH_NEIGHBOURS, _ffi.DEPTH_HISTOGRAM, _ffi.DEPTH_SEGMENT3, _ffi.DEPTH_PLANAR, _ffi.DEPTH_PARALLEL, _ffi.DEPTH_GLOBAL, _ffi.DEPTH_LOCAL,
               _ffi.DEPTH_OK]


def test_restatement_equals_the_frozen_oracle_with_default_parameters(oracle, capfd, monkeypatch):
    """Depths bit for bit, the ground plane bit for bit, and the reason histogram equal to the oracle's per-gate counts
    (ORACLE_DEPTH_STATS, read from stderr) on the scenes tests/test_depth.py uses."""
    monkeypatch.setenv("ORACLE_DEPTH_STATS", "1")
    lib_defaults = _ffi.DepthParams()
    _ffi.load().limo_depth_default_params(C.byref(lib_defaults))
    seen = np.zeros(10, int)
    for name, fr, labels in oracle_scenes():
        capfd.readouterr()
        do = oracle.depth_estimate(fr, use_ground_labels=labels)  # the oracle's own defaults: the ABI-6 part is zero
        stats = ORACLE_STATS.search(capfd.readouterr().err)
        assert stats, name
        for p in (oracle.depth_default_params(), lib_defaults):  # ... and the file's values there change nothing
            ref = dm.ref_estimate(fr, p, use_ground_labels=labels)
            assert np.array_equal(bits(ref["depth"]), bits(do)), name
            hist = np.bincount(ref["reasons"], minlength=10)
            assert [int(hist[g]) for g in STATS_ORDER] == [int(v) for v in stats.groups()], name
            assert hist[_ffi.DEPTH_PCA] == 0 and hist[_ffi.DEPTH_DEGENERATE] == len(do) - sum(int(v) for v in stats.groups())
            assert np.array_equal(ref["reasons"] == _ffi.DEPTH_OK, do > 0)
        seen += hist
        if labels:
            n_o, pl_o = oracle.ground_plane(fr)
            n_r, pl_r, _ = dm.ref_ground_plane(fr, lib_defaults)
            assert n_o == n_r and np.array_equal(pl_o, pl_r), name
    assert all(seen[g] > 0 for g in (_ffi.DEPTH_OK, _ffi.DEPTH_NEIGHBOURS, _ffi.DEPTH_SEGMENT3, _ffi.DEPTH_PLANAR, _ffi.DEPTH_PARALLEL)), seen


def test_restatement_equals_the_oracle_on_its_parameter_variants(oracle):
    fr = synth_lidar.make_frame(7)
    for changes in ({"ransac_plane_use_refinement": 0}, {"pixelarea_search_offset_x": 3, "pixelarea_search_offset_y": -2},
                    {"pixelarea_search_width": 14, "pixelarea_search_height": 20}, {"do_use_histogram_segmentation": 0},
                    {"treshold_depth_local_valuetype": 0, "treshold_depth_local_value": 0.2}, {"plane_estimator_use_mestimator": 0},
                    {"do_check_triangleplanar_condition": 0, "neighbors_count_min": 5}, {"ransac_seed": 99}, {"treshold_depth_max": 15.0}):
        p = dm.params_with(changes)
        assert np.array_equal(bits(dm.ref_estimate(fr, p)["depth"]), bits(oracle.depth_estimate(fr, params=p))), changes
    # plane_estimator_use_leastsquares is what plane_estimator_use_mestimator 0 has always done
    a = dm.ref_estimate(fr, dm.params_with({"plane_estimator_use_mestimator": 0, "plane_estimator_use_leastsquares": 1}))
    b = dm.ref_estimate(fr, dm.params_with({"plane_estimator_use_mestimator": 0}))
    assert np.array_equal(bits(a["depth"]), bits(b["depth"])) and np.array_equal(a["reasons"], b["reasons"])


# ----------------------------------------------------------------- independent checks of the modes (CPU, numpy, from the file)
def project(fr):
    """Pixels and camera-frame positions of the visible returns (numpy, the file's pinhole model)."""
    from limo_amd.synth import pose_to_Rt

    R, t = pose_to_Rt(np.asarray(fr["T_cam_lidar"], float))
    pc = fr["cloud"][:, :3].astype(np.float64) @ R.T + t
    pc = pc[pc[:, 2] > 0]
    u = fr["f"] * pc[:, 0] / pc[:, 2] + fr["cx"]
    v = fr["f"] * pc[:, 1] / pc[:, 2] + fr["cy"]
    inside = (u >= 0) & (u < fr["w"]) & (v >= 0) & (v < fr["h"])
    return u[inside], v[inside], pc[inside]


@pytest.mark.parametrize("tilt", [0.0, 0.01])
def test_pca_mode_recovers_the_depth_of_an_analytic_wall(tilt):
    """A 30x30 px window on the wall spreads the returns by +-0.25 m: the file's eigenvalue gates accept, and the depth is
    the plane's within the tolerance test_oracle_recovers_plane_depth_exactly uses.  In the file's own 6x9 px window the
    largest eigenvalue (variance along the window, ~0.002 m^2) stays below pca_treshold_3_abs_min = 0.005: PCA gate."""
    fr = wall_frame(tilt=tilt)
    pca = {"do_use_PCA": 1, "do_use_triangle_size_maximation": 0}
    ref = dm.ref_estimate(fr, dm.params_with(dict(pca, pixelarea_search_width=30, pixelarea_search_height=30)), use_ground_labels=False)
    assert (ref["reasons"] == _ffi.DEPTH_OK).all() and (ref["depth"] > 0).all()
    assert np.allclose(ref["depth"], expected_wall_depth(fr), rtol=2e-5)
    small = dm.ref_estimate(fr, dm.params_with(pca), use_ground_labels=False)
    assert (small["reasons"] == _ffi.DEPTH_PCA).all() and (small["depth"] == -1).all()
    # numpy's eigen-decomposition of the same scatter for one feature: same gate values, same depth
    u, v, pc = project(fr)
    fu, fv = fr["uv"][0].astype(np.float64)
    nb = pc[(np.abs(u - fu) <= 15) & (np.abs(v - fv) <= 15)]
    lam, vec = np.linalg.eigh(np.cov(nb.T, bias=True))
    assert lam[2] >= 0.005 and lam[2] <= 15 * lam[1] and lam[1] >= 1.5 * lam[0]
    n = vec[:, 0]
    ray = np.array([(fu - KITTI_CX) / KITTI_F, (fv - KITTI_CY) / KITTI_F, 1.0])
    assert abs((n @ nb.mean(0)) / (n @ ray) - ref["depth"][0]) < 1e-5 * ref["depth"][0]


def test_radius_mode_counts_agree_with_brute_force():
    fr = dm.small_frame(1, n_az=2000)
    p = dm.params_with({"neighbor_search_mode": 1})
    ref = dm.ref_estimate(fr, p)
    u, v, _ = project(fr)
    uv = fr["uv"].astype(np.float64)
    want = np.array([int((((u - fu) ** 2 + (v - fv) ** 2) <= 100.0).sum()) for fu, fv in uv])
    assert np.array_equal(ref["n_neighbours"], want) and want.max() > 20
    assert np.array_equal(ref["reasons"] == _ffi.DEPTH_NEIGHBOURS, want < 3)
    # radiusSearch_count_min is the radius search's key, neighbors_count_min the rectangle's
    more = dm.ref_estimate(fr, dm.params_with({"neighbor_search_mode": 1, "radiusSearch_count_min": 25, "neighbors_count_min": 1}))
    assert np.array_equal(more["reasons"] == _ffi.DEPTH_NEIGHBOURS, want < 25) and (want < 25).any() and (want >= 25).any()


def test_clamp_modes_return_exactly_the_bound():
    """The flat wall at 12 m: every return has z = 12 exactly, every feature's depth is 12 (within rounding)."""
    fr = wall_frame(tilt=0.0)
    n = len(fr["uv"])

    def run(**changes):
        return dm.ref_estimate(fr, dm.params_with(changes), use_ground_labels=False)

    hi = run(treshold_depth_mode=1, treshold_depth_max=10.0)  # 12 >= 10 -> 10; the local gate [6, 18] lets 10 pass
    assert (hi["depth"] == np.float32(10.0)).all() and (hi["reasons"] == _ffi.DEPTH_GLOBAL).all() and (hi["detail"] & dm.CLAMP_GLOBAL_HI).all()
    lo = run(treshold_depth_mode=1, treshold_depth_min=15.0)
    assert (lo["depth"] == np.float32(15.0)).all() and (lo["reasons"] == _ffi.DEPTH_GLOBAL).all() and (lo["detail"] & dm.CLAMP_GLOBAL_LO).all()
    rejected = run(treshold_depth_mode=0, treshold_depth_max=10.0)
    assert (rejected["depth"] == -1).all() and (rejected["reasons"] == _ffi.DEPTH_GLOBAL).all()
    # local bounds [zlo - v, zhi + v] with zlo = zhi = 12: v = -1 -> lo = 13 > 12: clamped up to 13
    up = run(treshold_depth_local_mode=1, treshold_depth_local_valuetype=0, treshold_depth_local_value=-1.0)
    assert (up["depth"] == np.float32(13.0)).all() and (up["reasons"] == _ffi.DEPTH_LOCAL).all() and (up["detail"] & dm.CLAMP_LOCAL_LO).all()
    # the global gate lifts 12 to 15, the local gate [11, 13] then takes it down to 13: the later gate's code
    down = run(treshold_depth_mode=1, treshold_depth_min=15.0, treshold_depth_local_mode=1, treshold_depth_local_valuetype=0, treshold_depth_local_value=1.0)
    assert (down["depth"] == np.float32(13.0)).all() and (down["reasons"] == _ffi.DEPTH_LOCAL).all()
    assert (down["detail"] & dm.CLAMP_LOCAL_HI).all() and (down["detail"] & dm.CLAMP_GLOBAL_LO).all()
    # global clamp, local gate still rejecting: 15 is outside [11, 13]
    mixed = run(treshold_depth_mode=1, treshold_depth_min=15.0, treshold_depth_local_valuetype=0, treshold_depth_local_value=1.0)
    assert (mixed["depth"] == -1).all() and (mixed["reasons"] == _ffi.DEPTH_LOCAL).all() and len(mixed["depth"]) == n


def test_corridor_keeps_the_band_returns_in_front_of_the_camera():
    fr = dm.small_frame(1)
    from limo_amd.synth import pose_to_Rt

    R, t = pose_to_Rt(np.asarray(fr["T_cam_lidar"], float))
    z = fr["cloud"][:, 2].astype(np.float64)
    x_cam = (fr["cloud"][:, :3].astype(np.float64) @ R.T + t)[:, 0]
    band = (z >= -3.5) & (z <= -1.0)
    for width in (12.0, 40.0):
        _, _, nb = dm.ref_ground_plane(fr, dm.params_with({"ransac_plane_use_camx_treshold": 1, "ransac_plane_treshold_camx": width}))
        assert nb == int((band & (np.abs(x_cam) <= width / 2)).sum()) and 0 < nb < band.sum()  # "width" is the full width
    assert dm.ref_ground_plane(fr, dm.params_with({}))[2] == band.sum()


def test_triangle_ground_patch_is_the_plane_of_the_largest_triangle():
    """Ground features of a sweep: where the patch is accepted the depth is that of the plane through the three patch
    points of largest area (numpy, itertools); elsewhere the sweep's plane answers."""
    import itertools

    fr = dm.small_frame(1)
    p = dm.params_with(dm.MODES["triangle_patch"])
    ref = dm.ref_estimate(fr, p)
    _, pl, _ = dm.ref_ground_plane(fr, p)
    u, v, pc = project(fr)
    checked = 0
    for k in np.flatnonzero((ref["detail"] & dm.PATCH_LOCAL) != 0)[:12]:
        fu, fv = fr["uv"][k].astype(np.float64)
        nb = pc[(np.abs(u - fu) <= 7) & (np.abs(v - fv) <= 10)]
        patch = nb[np.abs(nb @ pl[:3] + pl[3]) < 0.2]
        tri = max(itertools.combinations(range(len(patch)), 3), key=lambda t: np.linalg.norm(np.cross(patch[t[1]] - patch[t[0]], patch[t[2]] - patch[t[0]])))
        n = np.cross(patch[tri[1]] - patch[tri[0]], patch[tri[2]] - patch[tri[0]])
        ray = np.array([(fu - KITTI_CX) / KITTI_F, (fv - KITTI_CY) / KITTI_F, 1.0])
        depth = (n @ patch[tri[0]]) / (n @ ray)
        if ref["reasons"][k] == _ffi.DEPTH_OK:
            assert abs(depth - ref["depth"][k]) < 1e-5 * depth
            checked += 1
    assert checked >= 5


@pytest.mark.parametrize("mode", list(dm.MODES))
def test_mode_cases_take_every_new_exit(mode):
    """The cases of the GPU comparison below, on the CPU: each of them accepts features and takes every exit its mode adds
    (PCA gate, both sides of both clamping gates, corridor, triangle patch and its fallback), so that comparison cannot
    pass vacuously.  (The GPU test repeats the assertion on the reference values it compares against.)"""
    for seed in dm.SEEDS:
        fr = dm.small_frame(seed)
        p = dm.params_with(dm.MODES[mode])
        got = dm.exits_taken(mode, dm.ref_estimate(fr, p), fr, p)
        assert all(v > 0 for v in got.values()), (mode, seed, got)


def test_limo_stream_reads_the_parameter_file(tmp_path):
    """limo_stream --depth-params with the reference's file reproduces the committed 40-frame poses of the emulated backend
    (the file's values are the defaults); a file it cannot read is an error that names the line."""
    from test_kba_shim import run_limo_stream  # the command of the golden drive

    exe = emu_ffi.build_stream_app(gpu=False)
    poses = str(tmp_path / "poses.txt")
    out = run_limo_stream(exe, 40, 2000, poses, extra=["--depth-params", dm.GOLDEN_YAML])
    assert out["frames"] == 40 and out["depth_fraction"] > 0.3
    want = np.loadtxt(os.path.join(ROOT, "tests", "golden", "limo_stream_emulated_40_frames_poses.txt"))
    got = np.loadtxt(poses)
    assert want.shape == got.shape and np.abs(want - got).max() <= 1e-9, np.abs(want - got).max()
    bad = tmp_path / "bad.yaml"
    bad.write_text("%YAML:1.0\ndo_use_PCA: 0\npca_treshold: 3\n")
    r = subprocess.run([exe, "--frames", "2", "--depth-params", str(bad)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "bad.yaml:3" in r.stderr and "pca_treshold" in r.stderr


# ------------------------------------------------------------------------------------------------------------------ GPU
def gpu_equals_ref(ctx, fr, p, use_ground_labels=True):
    from limo_amd import ba

    ref = dm.ref_estimate(fr, p, use_ground_labels=use_ground_labels)
    dg = ba.depth_estimate(ctx, fr, params=p, use_ground_labels=use_ground_labels)
    rg = ba.depth_last_reasons(ctx, len(dg))
    assert np.array_equal(bits(dg), bits(ref["depth"])), "GPU and restatement differ in %d depths" % (bits(dg) != bits(ref["depth"])).sum()
    assert np.array_equal(rg, ref["reasons"]), "GPU and restatement differ in %d reason codes" % (rg != ref["reasons"]).sum()
    if use_ground_labels:
        n_g, pl_g = ba.depth_last_ground_plane(ctx, 0)
        n_r, pl_r, _ = dm.ref_ground_plane(fr, p)
        assert n_g == n_r and np.array_equal(pl_g, pl_r)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", [(m, s) for m in dm.MODES for s in dm.SEEDS])
def test_gpu_modes_match_the_restatement(ctx, mode, seed):
    """Depths, reason codes and the ground plane, bit for bit, no tolerance, no feature left out."""
    fr = dm.small_frame(seed)
    p = dm.params_with(dm.MODES[mode])
    ref = gpu_equals_ref(ctx, fr, p)
    got = dm.exits_taken(mode, ref, fr, p)
    assert all(v > 0 for v in got.values()), got


@pytest.mark.gpu
def test_gpu_reason_codes_of_the_default_path(ctx, oracle):
    from limo_amd import ba

    fr = dm.small_frame(5, n_az=2000)
    for labels in (True, False):
        ref = gpu_equals_ref(ctx, fr, ba.depth_default_params(), use_ground_labels=labels)
        assert np.array_equal(bits(ref["depth"]), bits(oracle.depth_estimate(fr, use_ground_labels=labels)))
        assert len(set(ref["reasons"].tolist())) >= 4
    # a struct whose ABI-6 part is zero (the frozen oracle's defaults) selects the same path
    dz = ba.depth_estimate(ctx, fr, params=oracle.depth_default_params())
    assert np.array_equal(bits(dz), bits(oracle.depth_estimate(fr)))


@pytest.mark.gpu
def test_gpu_radius_mode_beyond_64_neighbours(ctx):
    """4000 azimuth steps: a 10 px radius holds more than 64 returns for part of the features (the rectangle's cap)."""
    fr = dm.small_frame(2, n_az=4000)
    ref = gpu_equals_ref(ctx, fr, dm.params_with({"neighbor_search_mode": 1}))
    assert ref["n_neighbours"].max() > 64 and ref["n_neighbours"].max() <= 128 and (ref["depth"] > 0).any()


@pytest.mark.gpu
def test_gpu_modes_in_a_batch_of_unequal_frames(ctx):
    from limo_amd import ba

    frames = [dm.small_frame(11), dm.small_frame(12, n_az=900), dict(dm.small_frame(13))]
    frames[2]["uv"] = frames[2]["uv"][:150]
    frames[2]["is_ground"] = frames[2]["is_ground"][:150]
    for mode in ("combined", "pca"):
        p = dm.params_with(dm.MODES[mode])
        batch = ba.depth_estimate_batch(ctx, frames, params=p)
        reasons = [ba.depth_last_reasons(ctx, len(b), frame=k) for k, b in enumerate(batch)]
        for k, fr in enumerate(frames):
            ref = dm.ref_estimate(fr, p)
            assert np.array_equal(bits(batch[k]), bits(ref["depth"])) and np.array_equal(reasons[k], ref["reasons"]), (mode, k)
            assert (ref["depth"] > 0).any()
        with pytest.raises(ba.LimoError):
            ba.depth_last_reasons(ctx, len(batch[0]) + 1, frame=0)
        with pytest.raises(ba.LimoError):
            ba.depth_last_reasons(ctx, len(batch[0]), frame=3)


@pytest.mark.gpu
def test_gpu_refused_settings(ctx):
    """The three settings the library does not build and the three contradictory ones: their codes, the key in
    limo_last_error, and a context that still works."""
    from limo_amd import ba

    fr = dm.small_frame(1)
    uv = np.ascontiguousarray(fr["uv"], np.float32)
    cloud = np.ascontiguousarray(fr["cloud"], np.float32)
    T = np.ascontiguousarray(fr["T_cam_lidar"], np.float64)
    out = np.zeros(len(uv), np.float32)
    cases = [
        ({"do_use_depth_segmentation": 1}, _ffi.LIMO_ERR_UNSUPPORTED, "do_use_depth_segmentation"),
        ({"neighbor_search_mode": 1, "do_use_nearestNeighborSearch": 1}, _ffi.LIMO_ERR_UNSUPPORTED, "do_use_nearestNeighborSearch"),
        ({"plane_estimator_z_x_min_relation": 0.5}, _ffi.LIMO_ERR_UNSUPPORTED, "plane_estimator_z_x_min_relation"),
        ({"do_use_PCA": 1}, _ffi.LIMO_ERR_INVALID, "do_use_PCA"),
        ({"plane_estimator_use_leastsquares": 1}, _ffi.LIMO_ERR_INVALID, "plane_estimator_use_"),
        ({"neighbor_search_mode": 1, "do_use_radiusSearch": 0}, _ffi.LIMO_ERR_INVALID, "neighbor_search_mode"),
    ]
    for changes, code, key in cases:
        p = dm.params_with(changes, ba.depth_default_params())
        rc = ctx.lib.limo_depth_estimate(ctx.ptr, cloud.ctypes.data_as(_ffi.c_float_p), cloud.shape[0], T.ctypes.data_as(_ffi.c_double_p), fr["f"], fr["cx"],
                                         fr["cy"], fr["w"], fr["h"], uv.ctypes.data_as(_ffi.c_float_p), len(uv), None, C.byref(p), out.ctypes.data_as(_ffi.c_float_p))
        assert rc == code, changes
        assert key in ctx.lib.limo_last_error(ctx.ptr).decode(), changes
        with pytest.raises(ba.LimoError, match=key):
            ba.depth_estimate_begin(ctx, fr, params=p)
        with pytest.raises(ba.LimoError, match=key):
            ba.depth_estimate_batch(ctx, [fr, fr], params=p)
        gpu_equals_ref(ctx, fr, dm.params_with(dm.MODES["pca"]))  # the context stays usable
    # the nearest-neighbour flag is read in search mode 1 only
    gpu_equals_ref(ctx, fr, dm.params_with({"do_use_nearestNeighborSearch": 1, "pixelarea_search_width": 14, "pixelarea_search_height": 20}))


@pytest.mark.gpu
def test_gpu_frame_estimated_with_the_parameter_file(ctx):
    from limo_amd import ba

    fr = dm.small_frame(4, n_az=2000)
    want = ba.depth_estimate(ctx, fr)
    got = ba.depth_estimate(ctx, fr, params=load_depth_params(dm.GOLDEN_YAML))
    assert np.array_equal(bits(got), bits(want)) and (want > 0).any()
    assert np.array_equal(bits(ba.depth_estimate(ctx, fr, params=None)), bits(want))
