"""CPU: vrh_multi_volume_render_host -- the host build of include/visionaray_hip/detail/vrh_multi_volume.h -- against
every tests/golden/mv_<case>.npz: alpha, hit, tmin, the steps of every pixel and their total bit for bit, rgb to
rtol 1e-5 (the C library's powf need not round as the generator's did), mv_unshaded bit for bit in all four
channels.  The fixtures are frames of the reference's own multi-volume loop (tests/golden/multi_volume_ref.cpp,
run by make_multi_volume_golden.py); the conditions that generator enforces are checked again here.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_cases as MC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def host_frame(name):
    F = MC.load_frame(name)
    vox, tfs, filters, addresses, entries, k, cam = MC.frame_objects(F)
    return F, va.multi_volume_render_host(vox, tfs, entries, cam, k, filters, addresses)


@pytest.mark.parametrize("name", MC.FRAMES)
def test_host_render_equals_the_reference(name):
    F, got = host_frame(name)
    MC.check_frame(got, F, name, exact_rgb=name == "mv_unshaded")
    assert got["stats"] == {"rays": MC.FRAME_W * MC.FRAME_H, "steps": int(F["total_steps"][0]), "capped": 0}
    # vrh_multi_volume_count_host: the shaded samples are the reference's, and every sample belongs to a step
    assert got["shaded_samples"] == int(F["counters"][3]) and got["samples"] >= got["shaded_samples"] + int(F["counters"][4])
    assert got["samples"] >= int(F["total_steps"][0]) - int(F["counters"][2]) + int(F["counters"][1])


def test_fixture_conditions():
    with open(os.path.join(HERE, "golden", "multi_volume.json")) as f:
        recs = json.load(f)["frames"]
    assert sorted(recs) == sorted(MC.FRAMES)
    seen = {"miss": False, "two": 0, "none": 0, "shaded": 0, "zero_gradient": 0}
    for name in MC.FRAMES:
        F, rec = MC.load_frame(name), recs[name]
        hit, color, steps = F["hit"].astype(bool), F["color"], F["steps_px"].astype(np.int64)
        assert color.shape == (MC.FRAME_W * MC.FRAME_H, 4) and np.isfinite(color).all()
        assert int(steps.sum()) == int(F["total_steps"][0]) == rec["total_steps"] == int(F["counters"][0])
        assert np.all(color[~hit] == 0.0), "a miss leaves colour (0, 0, 0, 0)"
        assert int(steps.max()) < rec["cap"] and os.path.getsize(os.path.join(HERE, "golden", name + ".npz")) < (1 << 20)
        n = len(F["entries"])
        assert 1 <= n <= 32 and all(F["voxels_%d" % i].size <= 16 ** 3 for i in range(n))
        for i in range(n):
            m = F["entries"][i][31:44]                      # ca[3] ka cd[3] kd cs[3] ks exp
            assert np.all(m[4:7] * m[7] > 0.0), "kd * cd > 0 in every channel: no channel is a blinn term alone"
            assert np.all(F["transfunc_%d" % i] >= 0.0)
        seen["miss"] |= bool(hit.any() and (~hit).any())
        _, two, none, shaded, zero_gradient, cut = (int(c) for c in F["counters"])
        seen["two"] += two
        seen["none"] += none
        seen["shaded"] += shaded
        seen["zero_gradient"] += zero_gradient
        if name == "mv_formats":
            assert cut >= 0.05 * hit.sum() and hit.sum() - cut >= 0.05 * hit.sum()
            assert sorted(int(f) for f in F["vol_params"][:, 0]) == [0, 1, 2], "R8, R16 and R32F in one frame"
            assert len({tuple(int(x) for x in p[1:]) for p in F["vol_params"]}) == 3 and len({len(F["transfunc_%d" % i]) for i in range(3)}) == 3
            lin = F["entries"][1][15:31].reshape(4, 4).T[:3, :3]
            assert not np.allclose(np.linalg.norm(lin, axis=0), np.linalg.norm(lin, axis=0)[0]), "a non-uniform scale"
        if name == "mv_unshaded":
            assert shaded == 0 and zero_gradient == 0 and two > 0
            assert all(np.all(F["transfunc_%d" % i][:, 3] < F["kernel"][1]) for i in range(n))
        if name == "mv_inside":
            assert hit.all() and np.all(F["tmin"] < 0), "the eye inside a box, another box behind it"
        if name == "mv_gap":
            assert none > 0 and two == 0
    assert seen["miss"] and seen["two"] > 0 and seen["none"] > 0 and seen["shaded"] > 0 and seen["zero_gradient"] > 0


def test_the_example_case_is_the_examples_configuration():
    F = MC.load_frame("mv_example")
    assert len(F["entries"]) == 3 and list(F["kernel"]) == [np.float32(0.007), np.float32(0.1), np.float32(0.01)]
    assert float(F["cutoff"][0]) == 0.999
    k = va.multi_volume_kernel_desc(va.point_light((0.0, 0.0, 0.0)))                 # the defaults are the example's
    assert [k.dt, k.shade_alpha, k.gradient_delta] == [float(x) for x in F["kernel"]]
    assert k.opacity_cutoff == va.api.float_not_below(0.999)
    tf = [[0.0, 0.2, 0.8, 0.005], [1.0, 0.8, 0.0, 0.01], [0.0, 1.0, 0.0, 0.50], [1.0, 0.8, 0.0, 0.01], [1.0, 1.0, 1.0, 0.005]]
    assert np.array_equal(F["transfunc_0"], np.asarray(tf, np.float32))
    assert all(list(F["tf_params"][i]) == [0, 2] and list(F["vol_params"][i]) == [2, 1, 2, 2, 2] for i in range(3))
    s = float(np.sqrt(np.float32(0.5)))
    for i in range(3):
        e = F["entries"][i]
        assert list(e[0:15]) == [-1.0] * 3 + [1.0] * 3 + [1.0, -1.0, -1.0] + [1.0] * 3 + [2.0] * 3
        assert list(e[31:44]) == [np.float32(x) for x in [0.2] * 3 + [1.0] + [0.8] * 3 + [1.0] + [0.8] * 3 + [1.0, 128.0]]
        minv = e[15:31].reshape(4, 4).T                    # [row, col]
        assert np.allclose(np.abs(minv[:3, :3][np.abs(minv[:3, :3]) > 0.1]).min(), s, atol=1e-6), "a rotation by pi / 4"
        world = np.linalg.inv(minv.astype(np.float64))[:3, 3]
        assert np.allclose(world, [2.5 * i, 0.0, 0.0], atol=1e-6), "translated by 2.5 i along x"
    assert np.array_equal(F["light"][0:3], F["camera"][0:3]), "the light sits at the eye"


def test_single_volume_identity_equals_the_single_volume_march():
    """one volume under the identity transform with shade_alpha above every alpha: the two loops coincide (an
    identity Minv reproduces pos exactly, 0 + c leaves c), so every output equals vrh_volume_render_host's"""
    import vol_cases as VC
    for name in ("vol_r8_wrap", "vol_r16_mirror", "vol_r32f_16", "vol_box"):
        F = VC.load_frame(name)
        tf, k1, cam, filt, addr = VC.frame_objects(F)
        want = va.volume_render_host(F["voxels"], tf, cam, k1, filt, addr)
        entries = va.multi_volume_entries([(k1.box_min[:], k1.box_max[:])], [np.eye(4, dtype=np.float32)], [va.plastic()])
        entries[0].coord_sign[:], entries[0].coord_offset[:], entries[0].coord_extent[:] = k1.coord_sign[:], k1.coord_offset[:], k1.coord_extent[:]
        k = va.multi_volume_kernel_desc(va.point_light((0.0, 0.0, 0.0)), dt=k1.dt, shade_alpha=2.0)
        k.opacity_cutoff = k1.opacity_cutoff
        got = va.multi_volume_render_host([F["voxels"]], [tf], entries, cam, k, [filt], [addr])
        for key in ("color", "t", "prim_id", "steps_px"):
            assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), (name, key)
        assert got["stats"] == want["stats"]
