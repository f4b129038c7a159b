"""The five-point motion prior in the CPU tier: limo_amd/csrc/five_point_core.hpp - the statement the lanes of five_point.hip run -
against the host estimator limo_amd/kba/five_point.hpp, bit for bit (tests/cpp/test_five_point_core.cpp, a stand-alone program, also
built under -fsanitize=address,undefined): the minimal solver over 2400 random samples and the degenerate ones, and the chunked
pipeline of limo_five_point (all samples of a chunk, full inlier counts, the stopping rule afterwards) emulated on the host against
estimateMotion for match counts 5, 6, 64, 65, 300, chunk sizes 1, 7, 64, max_samples, and outlier shares 0.1, 0.3, 0.5."""
import os
import re
import subprocess

import pytest

import five_point_common as fpc
from limo_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_gives_the_host_estimators_bits(which):
    plain, san = fpc.build_unit()
    r = subprocess.run([plain if which == "plain" else san], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:]
    # the program checks these itself; stated here for the reader of a log
    m = re.search(r"minimal solver: (\d+) samples \((\d+) random\), \d+ models, (\d+) samples without a model, (\d+) with four or more", r.stdout)
    assert m and int(m.group(2)) >= 2000 and int(m.group(3)) >= 1 and int(m.group(4)) >= 1
    m = re.search(r"stopped within 64 samples: (\d+), later but below the cap: (\d+), at the cap: (\d+)", r.stdout)
    assert m and all(int(g) >= 1 for g in m.groups())


def test_structs_match_the_header():
    import ctypes as C

    src = open(os.path.join(ROOT, "include", "limo_hip.h")).read()
    for name in ("limo_five_point_params", "limo_five_point_motion", "limo_five_point_frame"):
        assert re.search(r"typedef struct %s \{" % name, src), name
    assert C.sizeof(_ffi.FivePointParams) == 24
    assert C.sizeof(_ffi.FivePointMotion) == 16 + 8 * 21
    assert C.sizeof(_ffi.FivePointFrame) == 32
    assert re.search(r"#define LIMO_ABI_VERSION 6\b", src)  # additive symbols: the version stays


def test_checker_is_the_host_estimator_and_repeats_itself():
    a, b = fpc.make_matches(3, 120, 0.3)
    r0, r1 = fpc.ref_estimate(a, b, seed=9), fpc.ref_estimate(a, b, seed=9)
    assert r0["ok"] and r0["raw"] == r1["raw"] and r0["inliers"] == int(r0["inlier"].sum()) and 60 <= r0["inliers"] <= 120
    assert abs(float((r0["t"] ** 2).sum()) - 1.0) < 1e-12 and r0["t"][2] < -0.9  # x_b = R x_a + t, the camera drives forward: t ~ (0, 0, -1)
    few = fpc.ref_estimate(a[:4], b[:4])
    assert not few["ok"] and few["samples"] == 0 and few["t"].tolist() == [0.0, 0.0, 1.0]
