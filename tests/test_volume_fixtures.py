"""CPU: vrh_volume_render_host -- the host build of the box clip and march of
include/visionaray_hip/detail/vrh_volume.h -- reproduces every tests/golden/vol_<case>.npz bit for bit: colour,
hit, tnear, the steps of every pixel and their total.  The fixtures are frames of the reference's own volume
loop (tests/golden/volume_ref.cpp, run by make_volume_golden.py); the conditions that generator enforces on
them are checked again here.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vol_cases as VC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def host_frame(name):
    F = VC.load_frame(name)
    tf, k, cam, filt, addr = VC.frame_objects(F)
    return F, va.volume_render_host(F["voxels"], tf, cam, k, filt, addr)


@pytest.mark.parametrize("name", VC.FRAMES)
def test_host_render_equals_the_reference(name):
    F, got = host_frame(name)
    hit = F["hit"].astype(bool)
    assert np.array_equal(got["prim_id"] != 0xFFFFFFFF, hit)
    assert np.all(got["prim_id"][hit] == 0)
    assert np.array_equal(got["t"][hit].view(np.uint32), F["tnear"][hit].view(np.uint32))
    assert np.all(got["t"][~hit] == -1.0)
    assert np.array_equal(got["steps_px"], F["steps_px"].astype(np.uint32))
    bad = np.flatnonzero(np.any(got["color"].view(np.uint32) != F["color"].view(np.uint32), axis=1))
    assert bad.size == 0, f"{name}: {bad.size} pixels differ, first {bad[0]}: {got['color'][bad[0]]} != {F['color'][bad[0]]}"
    assert got["stats"] == {"rays": VC.FRAME_W * VC.FRAME_H, "steps": int(F["total_steps"][0]), "capped": 0}


@pytest.mark.parametrize("name", VC.FRAMES)
def test_fixture_conditions(name):
    F = VC.load_frame(name)
    hit = F["hit"].astype(bool)
    color, steps = F["color"], F["steps_px"].astype(np.int64)
    assert color.shape == (VC.FRAME_W * VC.FRAME_H, 4) and np.isfinite(color).all()
    assert int(steps.sum()) == int(F["total_steps"][0])
    assert np.all(color[~hit] == 0.0) and np.all(steps[~hit] == 0), "a miss leaves colour (0, 0, 0, 0): no background"
    if name not in VC.EYE_RELATIVE:
        assert hit.any() and (~hit).any()
    if name == "vol_inside":
        assert hit.all() and np.all(F["tnear"] < 0), "the eye inside the box: the march starts behind the eye"
    if name == "vol_behind":
        assert hit.any() and np.all(F["tnear"][hit] < 0) and np.any(color[hit] != 0.0), "a box behind the eye is marched"
    cut = hit & (color[:, 3] >= float(F["cutoff"][0]))
    if name in VC.BOTH_ENDINGS:
        assert cut.sum() >= 0.05 * hit.sum() and (hit & ~cut).sum() >= 0.05 * hit.sum()
    k = F["kernel"]
    assert int(steps.max()) < VC.device_cap(k[0:3], k[3:6], k[15])
    with open(os.path.join(HERE, "golden", "volume.json")) as f:
        rec = json.load(f)["frames"][name]
    assert rec["total_steps"] == int(F["total_steps"][0]) and rec["hits"] == int(hit.sum()) and rec["cut"] == int(cut.sum())


def test_the_example_case_is_the_examples_configuration():
    F = VC.load_frame("vol_example")
    assert F["voxels"].shape == (2, 2, 2) and F["voxels"].dtype == np.float32 and len(F["transfunc"]) == 4
    assert list(F["vol_params"]) == [2, 0, 2, 2, 2] and list(F["tf_params"]) == [1, 2]
    k = va.volume_kernel_desc(((-1, -1, -1), (1, 1, 1)))                 # the defaults are the example's
    want = [*k.box_min, *k.box_max, *k.coord_sign, *k.coord_offset, *k.coord_extent, k.dt]
    assert np.array_equal(np.asarray(want, np.float32).view(np.uint32), F["kernel"].view(np.uint32))
    assert list(k.coord_sign) == [1.0, -1.0, -1.0] and list(k.coord_offset) == [1.0] * 3 and list(k.coord_extent) == [2.0] * 3
    assert float(F["cutoff"][0]) == 0.999


def test_float_cutoff_decides_as_the_double():
    """the smallest float not below the double c: w >= c and w >= that float agree on every float w around it"""
    for c in (0.999, 0.5, 1.0, 0.95, 1e-3):
        f = np.float32(va.api.float_not_below(c))
        assert float(f) >= c and float(np.nextafter(f, np.float32(-1.0))) < c
        w = f
        for _ in range(4):
            w = np.nextafter(w, np.float32(-1.0))
        for _ in range(9):
            assert (float(w) >= c) == bool(w >= f)
            w = np.nextafter(w, np.float32(2.0))
